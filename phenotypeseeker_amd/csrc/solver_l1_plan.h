// LDS placement of the bit-packed L1-logistic kernels (psk_logreg_l1_fit, solver.hip), as plain arithmetic on the problem
// shape and the form knobs: nothing here touches the device, so it can be read, compiled and checked on its own.
#pragma once
#include <cstddef>

// the form knobs of psk_logreg_l1_fit that bear on the placement (docs/KNOBS.md), already validated
struct psk_l1_knobs {
    bool no_cd_regs = false, no_gram = false, no_gram_global = false;   // PSK_NO_CD_REGS, PSK_NO_GRAM, PSK_NO_GRAM_GLOBAL
    bool set_min_p1 = false, set_reps = false;
    int min_p1 = 0, force_wmreg = 0, polish_reps = 0;   // PSK_GG_MIN_P1, PSK_FORCE_WMREG (0: n picks the register form), PSK_POLISH_REPS
};

// the placement fields of psk_l1_bits_launch, and the LDS bytes of the Gram-in-global form's own arrays (0: another form)
struct psk_l1_placement {
    int f_lds = 0, s_lds = 0, c_lds = 0, q_doubles = 0, gg_sl = 0, polish_reps = 0, wmreg = 0, all_lds = 0;
    size_t gg_stride = 0, gg_lds = 0, lds_bytes = 0;
};

// the kernels' static LDS (cooperation state of the bit-packed kernel: ~7 KB) comes on top
constexpr size_t PSK_L1_LDS_MAX = 160 * 1024 - 8192;

// the five feature arrays, and with them the active list of the bit-packed kernel
inline size_t psk_l1_feature_bytes(int p) { return 5 * (size_t)(p + 1) * 8; }
inline size_t psk_l1_feature_bytes_bits(int p) { return psk_l1_feature_bytes(p) + (((size_t)(p + 1) + 1) / 2) * 8; }
inline int psk_l1_wmreg_of(int W) { return W <= 16 ? 16 : W <= 32 ? 32 : 64; }

// More coordinates than the LDS Gram block takes (192): the Gram matrix of a fit in global memory, f32, a column
// per slot (gg_run).  Its LDS arrays (slot parameters, ring, D in operand order, orders, flags) take the place of
// the Gram block; the feature arrays must be in LDS beside them.
// Returns gg_sl (slots of a column), gg_stride (floats of a fit's matrix) and gg_lds when the form is wanted, else zeros.
inline psk_l1_placement psk_l1_gg_wanted(int n, int p, int W, int n_fits, const psk_l1_knobs &k, int coop_waves)
{
    psk_l1_placement g;
    const int P1 = p + 1, wmreg_h = k.no_cd_regs ? 0 : psk_l1_wmreg_of(W);
    // up to 192 columns the LDS Gram form (exact f64 Hessian, columns built sample by sample) keeps the designs with
    // fewer than 1,024 samples: its builds are cheap there and an ill-conditioned fit at a tight tolerance converges in
    // fewer Newton steps than with the f32 / bf16-split Q of the global form (256 x 150 near-duplicates at tol = 1e-7:
    // inside 300 steps against not); from 1,024 samples on the global form is 3-10 x faster (2048 x 169 grid 0.27 ->
    // 0.03 s, 2000 x 150: 0.14 -> 0.012 s)
    const int gg_min_p1 = k.set_min_p1 ? k.min_p1 : (n >= 1024 ? 64 : 192);
    if (!(P1 > gg_min_p1 && P1 <= 1024 && wmreg_h > 0 && coop_waves == 4 && !k.no_gram && !k.no_gram_global)) return g;
    const size_t sl = 256 * (((size_t)P1 + 255) / 256), np_h = (size_t)W * 64;
    // (+ the build's tables / wave 3's counters, + the owners' column buffers)
    const size_t need = (4 * sl + np_h + sl / 2 + sl / 4 + sl / 8) * 8 + 8192 + 16384, stride = (((size_t)P1 + 15) / 16 * 16) * sl;
    if (psk_l1_feature_bytes_bits(p) + need <= PSK_L1_LDS_MAX && (size_t)n_fits * stride * 4 <= ((size_t)32 << 30)) {
        g.gg_sl = (int)sl; g.gg_stride = stride; g.gg_lds = need;
    }
    return g;
}

// LDS budget of the bit-packed kernel.  The inner QP works on the Gram block, the per-feature arrays and the
// active list only, so those come first; the five sample arrays are streamed (coalesced) once per Newton
// step and line-search trial and move to global scratch when they do not fit beside the Gram block of the
// problem (thousands of samples: 5 x 2048 doubles are 80 KiB); the column bit words take what is left.
// (With the sample arrays first, a 2048-sample fit with 170 distinct patterns had room for 79 Gram columns,
// fell back to the array-form descent and took 0.5 s instead of 0.02 s, r01.)
// `L`: what psk_l1_gg_wanted returned when the Gram matrices could be allocated too, else a default-made record.
inline psk_l1_placement psk_l1_place(int p, int W, const psk_l1_knobs &k, psk_l1_placement L)
{
    const size_t sbytes = 5 * ((size_t)W * 64) * 8, fa = psk_l1_feature_bytes_bits(p), cbytes = (size_t)(p + 1) * W * 8;
    const bool gram = !k.no_gram && L.gg_sl == 0;
    const size_t pq = (size_t)(p + 1) < 192 ? (size_t)(p + 1) : 192;   // Gram columns the kernel can use
    const size_t need_q = gram ? pq * (pq + 1) / 2 * 8 : 0;             // its packed triangle
    size_t left = PSK_L1_LDS_MAX - L.gg_lds;
    L.f_lds = fa <= left ? 1 : 0; left -= L.f_lds ? fa : 0;
    // sample arrays: all five when they fit beside the whole Gram block; else only the two hot ones (tau, D) if
    // THAT makes room for the whole Gram block (thousands of samples, up to ~170 distinct patterns: the Gram form
    // with its accelerator converges where the array form runs into its sweep limit, r01: 2048 x 170, objective sum
    // of the grid 8.051e6 against 8.153e6, 0.73 s against 1.06 s); else all five again with a partial Gram block in
    // what is left (the previous behaviour); the hot ones alone when five do not fit at all
    const size_t hot_b = sbytes / 5 * 2;
    if (sbytes + need_q <= left) L.s_lds = 3;
    else if (gram && hot_b + need_q <= left) L.s_lds = 1;
    else if (sbytes <= left) L.s_lds = 3;
    else L.s_lds = hot_b <= left ? 1 : 0;
    const size_t s_in_lds = L.s_lds == 3 ? sbytes : (L.s_lds == 1 ? hot_b : 0);
    left -= s_in_lds;
    // the Gram block: up to the packed triangle of 192 features (a 64 x 64 or 128 x 128 square is preferred by the
    // kernel when it fits), before the column words
    size_t q_doubles = 0;
    if (gram) {
        const size_t square = pq <= 64 ? 64 * 64 : (pq <= 128 ? 128 * 128 : 0);
        q_doubles = need_q / 8;
        if (square * 8 <= left && square > q_doubles) q_doubles = square;
        if (q_doubles * 8 > left) q_doubles = left / 8;
        if (q_doubles < 36) q_doubles = 0;
    }
    left -= q_doubles * 8;
    L.c_lds = cbytes <= left ? 1 : 0; left -= L.c_lds ? cbytes : 0;
    if (gram && left >= 8) {   // leftover goes to the Gram block too (a square layout may now fit)
        const size_t most = (size_t)192 * 193 / 2;
        size_t more = q_doubles + left / 8;
        if (more > most) more = most;
        q_doubles = more;
    }
    if (L.gg_sl) q_doubles = L.gg_lds / 8;
    L.q_doubles = (int)q_doubles;
    L.lds_bytes = s_in_lds + q_doubles * 8 + (L.f_lds ? fa : 0) + (L.c_lds ? cbytes : 0);
    L.all_lds = L.f_lds && L.s_lds == 3 && L.c_lds && q_doubles > 0;
    // polishes in a row while signs change; negative (the Gram-global form's default): as many as the descent has needed
    // sweeps when the accelerator is called (32, 64, 128), at most that many -- the 2048 x 169 grid 0.105 -> 0.031 s, the
    // 2048 x 907 grid 0.236 -> 0.245 s against a fixed 64
    L.polish_reps = k.set_reps ? k.polish_reps : (L.gg_sl ? -128 : 64);
    L.wmreg = k.no_cd_regs ? 0 : k.force_wmreg ? k.force_wmreg : psk_l1_wmreg_of(W);
    return L;
}
