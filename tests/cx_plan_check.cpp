// Stand-alone check of csrc/chi2_plan.h, the host's decisions about an exception-coded chi2 scan (run by
// tests/test_cx_make_plan_host.py; no GPU, no library): which kernel form cx_make_plan picks, that the launch shape it
// returns for each of the three forms makes the kernels' index arithmetic visit every slot pair and every side-matrix row
// exactly once within the bound that sizes the result segments, and the plan of the flagship scan.  Integers and
// booleans throughout: no tolerance.
#include "../phenotypeseeker_amd/csrc/chi2_plan.h"

#include <cmath>
#include <cstdio>

static long n_checks = 0, n_fail = 0;
#define CHECK(cond, ...)                                          \
    do {                                                          \
        n_checks++;                                               \
        if (!(cond)) {                                            \
            if (n_fail++ < 20) { printf("FAIL %s:%d %s  ", __FILE__, __LINE__, #cond); printf(__VA_ARGS__); printf("\n"); } \
        }                                                         \
    } while (0)

static const uint64_t FLAG_M = 22950458, FLAG_N_OV = 1951321;

static double bonferroni_thr() { return -2.0 * log(0.05 / (double)FLAG_M); }

static CxPlanKey make_key(uint64_t M, uint64_t n_ov, int cpr, uint64_t cap, double thr, int side_kernel, int pc_filter)
{
    CxPlanKey k;
    k.M = M; k.n_ov = n_ov; k.cap = cap; k.side_cap = cap; k.pc_cap = cap;
    memcpy(&k.thr_bits, &thr, 8);
    k.n_samples = cpr == 1 ? 128 : 256;
    k.n1 = k.n0 = k.n_samples / 2;
    k.cpr = cpr;
    k.min_samples = 2; k.max_samples = k.n_samples - 2;
    k.side_kernel = side_kernel; k.pc_filter = pc_filter;
    return k;
}

// ---- form selection ----------------------------------------------------------------------------------------------------
static void check_forms()
{
    // popcounts 20 and 240 cannot pass the Bonferroni scan of 128 + 128 samples, 100 can (the flagship check below pins the range)
    struct { const char *name; uint64_t at20, at100, at240; } hists[3] = {{"all", 0, 1000, 0}, {"some", 400, 600, 0}, {"none", 600, 0, 400}};
    const double thrs[2] = {0.0, bonferroni_thr()};
    for (int t = 0; t < 2; t++)
        for (int side = 0; side < 2; side++)
            for (int pcf = 0; pcf < 2; pcf++)
                for (int h = 0; h < 3; h++) {
                    std::vector<uint64_t> hist(257, 0);
                    hist[20] = hists[h].at20; hist[100] = hists[h].at100; hist[240] = hists[h].at240;
                    const uint64_t n_ov = hists[h].at20 + hists[h].at100 + hists[h].at240;
                    const CxPlanKey key = make_key(100000, n_ov, 2, 2048, thrs[t], side, pcf);
                    const CxPlan pl = cx_make_plan(key, hist.data(), hist.size());
                    // today's rules, from the two plans themselves
                    const ScanCuts K = plan_cuts(key.n1, key.n0, key.min_samples, key.max_samples, thrs[t]);
                    uint32_t mask; uint64_t corner[2], feas[4];
                    cx_plan(K, key.n_samples, &mask, corner);
                    cx_pc_plan(K, key.n_samples, feas);
                    uint64_t rf = 0;
                    for (int pc = 0; pc < 256; pc++) if ((feas[pc >> 6] >> (pc & 63)) & 1) rf += hist[pc];
                    CHECK((mask == 0) == (t == 1), "thr %g: class mask %#x", thrs[t], mask);   // thr 0: every class; Bonferroni: none
                    Chi2Form want = Chi2Form::CxMixed;
                    if (side && mask == 0) want = pcf && rf < n_ov ? Chi2Form::CxSidePc : Chi2Form::CxSide;
                    CHECK(pl.valid && pl.form == want, "thr %g side %d filter %d hist %s: form %d, want %d", thrs[t], side, pcf, hists[h].name, (int)pl.form, (int)want);
                    CHECK(pl.class_mask == mask && pl.corner[0] == corner[0] && pl.corner[1] == corner[1], "plan differs from cx_plan");
                    if (t == 1 && side) {   // and what the rules come to, spelled out
                        const Chi2Form lit = !pcf || h == 0 ? Chi2Form::CxSide : Chi2Form::CxSidePc;
                        CHECK(pl.form == lit, "Bonferroni, side kernel on, filter %d, hist %s: form %d", pcf, hists[h].name, (int)pl.form);
                        if (pcf) CHECK(pl.rows_feasible == hists[h].at100, "rows_feasible %llu", (unsigned long long)pl.rows_feasible);
                    }
                    if (!(side && mask == 0 && pcf)) CHECK(pl.rows_feasible == n_ov && pl.feas[0] == ~0ull && pl.feas[3] == ~0ull, "unfiltered plan: all rows feasible");
                    CHECK(pl.key == key, "the plan records its key");
                }
}

// ---- the sweeps --------------------------------------------------------------------------------------------------------
struct Sweep {
    std::vector<uint8_t> seen;
    std::vector<uint64_t> per_block;
    uint64_t n;
    Sweep(uint64_t n_, uint64_t blocks) : seen(n_, 0), per_block(blocks, 0), n(n_) {}
    void visit(uint64_t block, uint64_t first, uint64_t count, uint64_t weight = 1)   // items [first, first + count) below n
    {
        for (uint64_t i = first; i < first + count && i < n; i++) { seen[i]++; per_block[block] += weight; }
    }
    bool once() const { for (uint8_t s : seen) if (s != 1) return false; return true; }
    uint64_t most() const { uint64_t m = 0; for (uint64_t v : per_block) m = std::max(m, v); return m; }
};

static void check_sweep(const CxPlan &pl, const char *what)
{
    const CxPlanKey &k = pl.key;
    const uint64_t W = CX_WAVES, rpw = 64 / (uint64_t)k.cpr;
    uint64_t rows_per_block = 0;
    Sweep rows(k.n_ov, pl.grid), pairs((k.M + 1) / 2, pl.grid);
    if (pl.form == Chi2Form::CxMixed) {   // chi2_scan_kernel_cx
        rows_per_block = cx_mixed_shape(k.M, k.n_ov, k.cpr, k.cap, pl.class_mask != 0).rows_per_block;
        const uint64_t n_pairs = (k.M + 1) / 2, batch = 64 * (uint64_t)CX_UNROLL;
        for (uint64_t b = 0; b < pl.slot_blocks; b++)
            for (uint64_t w = 0; w < W; w++)
                for (uint64_t p0 = (b * W + w) * batch; p0 < n_pairs; p0 += (uint64_t)pl.slot_blocks * W * batch) pairs.visit(b, p0, batch, 2);
        const uint64_t n_steps = (k.n_ov + rpw - 1) / rpw;
        for (uint64_t b = 0; b < pl.ov_blocks; b++)
            for (uint64_t w = 0; w < W; w++)
                for (uint64_t s0 = (b * W + w) * CX_UNROLL; s0 < n_steps; s0 += (uint64_t)pl.ov_blocks * W * CX_UNROLL) rows.visit(pl.slot_blocks + b, s0 * rpw, CX_UNROLL * rpw);
        if (pl.class_mask) CHECK(pairs.once(), "%s: slot pairs", what);
    } else if (pl.form == Chi2Form::CxSide) {   // chi2_scan_kernel_cx_side
        rows_per_block = cx_side_shape(k.n_ov, k.cpr, k.side_cap).rows_per_block;
        const uint64_t n_steps = (k.n_ov + rpw - 1) / rpw, stride = (uint64_t)pl.grid * W * CX_SIDE_UNROLL;
        for (uint64_t b = 0; b < pl.grid; b++)
            for (uint64_t w = 0; w < W; w++)
                for (uint64_t s0 = (b * W + w) * CX_SIDE_UNROLL; s0 < n_steps; s0 += stride) rows.visit(b, s0 * rpw, CX_SIDE_UNROLL * rpw);
    } else {   // chi2_scan_kernel_cx_side_pc
        rows_per_block = cx_pc_shape(k.n_ov, k.pc_cap).rows_per_block;
        const uint64_t batch = 64 * (uint64_t)CX_PC_UNROLL, n_batches = (k.n_ov + batch - 1) / batch;
        for (uint64_t b = 0; b < pl.grid; b++)
            for (uint64_t w = 0; w < W; w++)
                for (uint64_t i = b * W + w; i < n_batches; i += (uint64_t)pl.grid * W) rows.visit(b, i * batch, batch);
    }
    CHECK(rows.once(), "%s: side rows", what);
    std::vector<uint64_t> both(pl.grid);
    for (uint32_t b = 0; b < pl.grid; b++) both[b] = rows.per_block[b] + pairs.per_block[b];
    uint64_t most = 0;
    for (uint64_t v : both) most = std::max(most, v);
    CHECK(most <= rows_per_block, "%s: a workgroup visits %llu rows, bound %llu", what, (unsigned long long)most, (unsigned long long)rows_per_block);
    CHECK(pl.grid >= 256, "%s: grid %u", what, pl.grid);
    CHECK((uint64_t)pl.slot_blocks + pl.ov_blocks <= pl.grid, "%s: %u + %u workgroups of %u", what, pl.slot_blocks, pl.ov_blocks, pl.grid);
    CHECK((pl.slot_blocks == 0) == (pl.class_mask == 0), "%s: slot_blocks %u, class mask %#x", what, pl.slot_blocks, pl.class_mask);
    CHECK(pl.seg_cap == result_seg_cap(pl.grid, rows_per_block), "%s: seg_cap %llu", what, (unsigned long long)pl.seg_cap);
    // ... and, without the shape functions: a segment holds what the workgroups that map to it (blockIdx % CX_NSEG) visit
    std::vector<uint64_t> per_seg(CX_NSEG, 0);
    for (uint32_t b = 0; b < pl.grid; b++) per_seg[b % CX_NSEG] += both[b];
    uint64_t seg_most = 0;
    for (uint64_t v : per_seg) seg_most = std::max(seg_most, v);
    CHECK(seg_most <= pl.seg_cap, "%s: a segment's workgroups visit %llu rows, seg_cap %llu", what, (unsigned long long)seg_most, (unsigned long long)pl.seg_cap);
}

static void check_sweeps()
{
    const uint64_t Ms[] = {0, 1, 2, 129, 1000003}, caps[] = {256, 2048, 4096};
    // (mixed with every class, mixed with none, side, side by popcount) x the sizes
    struct { const char *name; double thr; int side, pcf; Chi2Form form; } forms[4] = {
        {"mixed, every class", 0.0, 0, 0, Chi2Form::CxMixed}, {"mixed, no class", bonferroni_thr(), 0, 0, Chi2Form::CxMixed},
        {"side", bonferroni_thr(), 1, 0, Chi2Form::CxSide}, {"side by popcount", bonferroni_thr(), 1, 1, Chi2Form::CxSidePc}};
    for (int f = 0; f < 4; f++)
        for (int cpr = 1; cpr <= 2; cpr++) {
            // rows of one wave batch of this form: one batch per wave of 256 workgroups, one less and one more
            const uint64_t batch = f < 2 ? CX_UNROLL * 64 / cpr : f == 2 ? CX_SIDE_UNROLL * 64 / cpr : 64 * CX_PC_UNROLL;
            const uint64_t one_each = 256 * CX_WAVES * batch;
            const uint64_t n_ovs[] = {0, 1, 63, 64, 65, one_each - 1, one_each, one_each + 1, 100001};
            for (uint64_t M : Ms)
                for (uint64_t n_ov : n_ovs)
                    for (uint64_t cap : caps) {
                        std::vector<uint64_t> hist(257, 0);
                        hist[20] = n_ov;   // a popcount no Bonferroni scan lets through: the filtered form whenever there are rows
                        const CxPlan pl = cx_make_plan(make_key(M, n_ov, cpr, cap, forms[f].thr, forms[f].side, forms[f].pcf), hist.data(), hist.size());
                        char what[160];
                        snprintf(what, sizeof what, "%s, M %llu, n_ov %llu, cpr %d, cap %llu", forms[f].name, (unsigned long long)M, (unsigned long long)n_ov, cpr, (unsigned long long)cap);
                        const Chi2Form want = f == 3 && n_ov == 0 ? Chi2Form::CxSide : forms[f].form;   // no rows: nothing to filter
                        CHECK(pl.form == want, "%s: form %d", what, (int)pl.form);
                        check_sweep(pl, what);
                    }
        }
}

// ---- the flagship scan ---------------------------------------------------------------------------------------------------
static void check_flagship()
{
    std::vector<uint64_t> hist(257, 0);
    hist[35] = 1000; hist[221] = 700; hist[128] = 36;            // 1,736 rows inside [35, 221] ...
    hist[34] = 1000000; hist[222] = FLAG_N_OV - 1736 - 1000000;   // ... and the rest just outside
    CxPlanKey key = make_key(FLAG_M, FLAG_N_OV, 2, 256 * 16, bonferroni_thr(), 1, 1);
    key.side_cap = key.pc_cap = 256 * 8;
    const CxPlan pl = cx_make_plan(key, hist.data(), hist.size());
    CHECK(pl.form == Chi2Form::CxSidePc, "form %d", (int)pl.form);
    CHECK(pl.rows_feasible == 1736, "rows_feasible %llu", (unsigned long long)pl.rows_feasible);
    for (int pc = 0; pc < 256; pc++)
        CHECK((((pl.feas[pc >> 6] >> (pc & 63)) & 1) != 0) == (pc >= 35 && pc <= 221), "popcount %d", pc);
    const cx_side_shape_t sh = cx_pc_shape(FLAG_N_OV, key.pc_cap);
    CHECK(pl.grid == sh.blocks && pl.ov_blocks == sh.blocks && pl.slot_blocks == 0, "grid %u, cx_pc_shape %u", pl.grid, sh.blocks);
    CHECK(pl.seg_cap == result_seg_cap(sh.blocks, sh.rows_per_block), "seg_cap %llu", (unsigned long long)pl.seg_cap);
    CHECK(pl.class_mask == 0, "class mask %#x", pl.class_mask);
}

int main()
{
    check_forms();
    check_sweeps();
    check_flagship();
    printf("%ld checks, %ld failures\n", n_checks, n_fail);
    return n_fail ? 1 : 0;
}
