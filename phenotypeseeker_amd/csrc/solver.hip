// a10: the two L1 estimators the reference fits behind GridSearchCV (modeling.py:994-1014,
// :1075-1085, :1208-1216), as batched HIP solvers: every (grid value, CV fold) pair and the final
// refit is an independent small problem (N <= a few thousand samples x <= ~1000 selected k-mers),
// so one workgroup solves one fit and all fits of a grid search run in ONE launch.
//
//   logreg_newglmnet_*  liblinear's L1R_LR objective  ||w||_1 + |b| + C sum log(1+exp(-y(w.x+b)))
//                     (intercept = penalised constant-1 feature) by the improved GLMNET scheme liblinear
//                     itself uses: outer Newton steps, inner coordinate descent with shrinking on the
//                     quadratic model, one line search per outer step; a bit-packed form for 0/1 designs.
//                     With PI = false the same without |b|, the free intercept of psk_logreg_l1_free_fit (saga's objective).
//   lasso_kernel      (1/2n)||y - Xw - b||^2 + alpha ||w||_1, unpenalised intercept, cyclic
//                     coordinate descent on the centred problem.  With EN = true the elastic net of psk_enet_fit (f14):
//                     + 1/2 alpha (1 - l1_ratio) ||w||^2, the L1 weight alpha l1_ratio.
//
// Layout: XT[p][n] float (column-major: one k-mer's samples are contiguous), shared by all fits and
// L2-resident; per fit the linear predictor / residual lives in LDS (global scratch beyond 4096 samples).
// Latency-bound, f64 VALU; the roofline that matters for this stage is wall-clock, not bandwidth
// (DESIGN.md).  The host removes duplicated columns first (model.GridSearch): k-mers of one gene share
// one presence pattern, and an L1 optimum may put a pattern's weight on any one of its copies.
#include <algorithm>

#include "solver_common.h"
#include "solver_host.h"
#include "solver_l1_plan.h"

namespace {

// L1 logistic regression by the improved GLMNET scheme (Yuan, Ho & Lin, JMLR 2012 -- the method behind
// liblinear's L1R_LR solver, which is what the reference's LogisticRegression(penalty='l1',
// solver='liblinear') runs): outer Newton iterations build a quadratic model from cached
// tau_i = C/(1+exp(w.x_i)) and D_i = C exp(w.x_i)/(1+exp(w.x_i))^2; an inner cyclic coordinate descent
// with shrinking solves the model WITHOUT any transcendental per coordinate; one Armijo line search per
// outer iteration (<= 20 halvings) needs exp/log once per sample.  Same stopping rule as liblinear:
// ||violation||_1 <= tol * min(#pos, #neg)/l * ||violation at w = 0||_1.
// Per-fit state: five feature arrays (w, w+d, diag H, grad, sum of C*x over the y=-1 rows) and five sample
// arrays (exp(w.x), its trial value, tau, D, x.d), in LDS when they fit (up to 160 KiB per workgroup).
// PI (here and in logreg_newglmnet_bits_kernel): the intercept is penalised -- liblinear's objective, psk_logreg_l1_fit.  With
// PI = false it is free (psk_logreg_l1_free_fit): its subgradient term is 0 in the violations, in the shrinking tests (which
// then never pass for it) and in the inner step (-G / H, no soft threshold), and it is left out of the line search's ||w||_1.
// A template parameter: the penalised instances compile to what they were.
#define FLD(ptr) (f_lds ? *(ptr) : lane0_load((ptr), lane))
template <bool PI>
__global__ __launch_bounds__(SV_THREADS) void logreg_newglmnet_kernel(
    const float *__restrict__ XT, const int8_t *__restrict__ ypm, const int32_t *__restrict__ fold, int n, int p,
    const double *__restrict__ fit_param, const int32_t *__restrict__ fit_fold, double tol, int max_newton,
    double *__restrict__ coef, double *__restrict__ icpt, int32_t *__restrict__ iters, double *__restrict__ work,
    int32_t *__restrict__ iwork, const int f_lds, const int s_lds)
{
    extern __shared__ double sm[];
    const int fit = blockIdx.x, lane = threadIdx.x;
    const double C = fit_param[fit];
    const int tf = fit_fold[fit];
    const int P1 = p + 1;
    double *gw = work + (size_t)fit * (5 * (size_t)P1 + 5 * (size_t)n);
    double *F = f_lds ? sm : gw;
    double *S = s_lds ? (sm + (f_lds ? 5 * P1 : 0)) : (gw + 5 * (size_t)P1);
    double *w = F, *wpd = F + P1, *Hd = F + 2 * P1, *Gr = F + 3 * P1, *xjneg = F + 4 * P1;
    double *ewx = S, *ewxn = S + n, *tau = S + 2 * (size_t)n, *D = S + 3 * (size_t)n, *xTd = S + 4 * (size_t)n;
    int32_t *act = iwork + (size_t)fit * P1;
    const double nu = 1e-12, sigma = 0.01;

    double npos = 0, nneg = 0;
    for (int i = lane; i < n; i += SV_THREADS) {
        ewx[i] = 1.0; tau[i] = C * 0.5; D[i] = C * 0.25; xTd[i] = 0.0;
        if (fold[i] != tf) { if (ypm[i] > 0) npos += 1; else nneg += 1; }
    }
    npos = psk_wave_sum_f64_dpp(npos);
    nneg = psk_wave_sum_f64_dpp(nneg);
    const double l = npos + nneg;
    double mn = npos < nneg ? npos : nneg;
    if (mn < 1.0) mn = 1.0;
    const double eps = tol * mn / (l > 0 ? l : 1.0);
    for (int j = 0; j < P1; j++) {  // feature arrays are written by lane 0 only (see lane0_load)
        const float *col = XT + (size_t)j * n;
        double sneg = 0.0;
        for (int i = lane; i < n; i += SV_THREADS)
            if (fold[i] != tf && ypm[i] < 0) sneg += C * ((j < p) ? (double)col[i] : 1.0);
        sneg = psk_wave_sum_f64_dpp(sneg);
        if (lane == 0) { w[j] = 0.0; wpd[j] = 0.0; xjneg[j] = sneg; act[j] = j; }
    }
    double w_norm = 0.0, Gmax_old = 1e300, Gnorm1_init = -1.0, inner_eps = 1.0;
    uint32_t rng = ((uint32_t)fit + 1u) * 2654435761u | 1u;  // per-fit xorshift state of the sweep permutations (lane 0's copy counts)
    int newton = 0, floor_steps = 0;   // floor_steps: Newton steps in a row taken inside the line search's rounding noise
    double Gbest = 1e300;              // the smallest violation of the fit so far
    double zmin = 1e-12;               // coordinate steps below it are skipped, as liblinear skips them
    for (newton = 0; newton < max_newton; newton++) {
        double Gmax_new = 0.0, Gnorm1_new = 0.0;
        int active = P1;
        for (int sidx = 0; sidx < active; sidx++) {
            const int j = __builtin_amdgcn_readfirstlane(lane == 0 ? act[sidx] : 0);
            const float *col = XT + (size_t)j * n;
            double hd = 0.0, tmp = 0.0;
            for (int i = lane; i < n; i += SV_THREADS) {
                if (fold[i] == tf) continue;
                const double x = (j < p) ? (double)col[i] : 1.0;
                if (x == 0.0) continue;
                hd += x * x * D[i];
                tmp += x * tau[i];
            }
            hd = psk_wave_sum_f64_dpp(hd) + nu;
            tmp = psk_wave_sum_f64_dpp(tmp);
            const double grad = -tmp + FLD(&xjneg[j]);
            const double wj = FLD(&w[j]);
            const double pen = (PI || j < p) ? 1.0 : 0.0;   // (PI false: the intercept, coordinate p, is free)
            const double Gp = grad + pen, Gn = grad - pen;
            double viol = 0.0;
            if (wj == 0.0) {
                if (Gp < 0) viol = -Gp;
                else if (Gn > 0) viol = Gn;
                else if (Gp > Gmax_old / l && Gn < -Gmax_old / l) {  // outer-level shrinking
                    active--;
                    if (lane == 0) { const int32_t t = act[sidx]; act[sidx] = act[active]; act[active] = t; }
                    sidx--;
                    continue;
                }
            } else if (wj > 0) viol = fabs(Gp);
            else viol = fabs(Gn);
            if (lane == 0) { Hd[j] = hd; Gr[j] = grad; }
            if (viol > Gmax_new) Gmax_new = viol;
            Gnorm1_new += viol;
        }
        if (newton == 0) Gnorm1_init = Gnorm1_new;
        const bool progressed = Gnorm1_new < 0.9 * Gbest;
        if (Gnorm1_new < Gbest) Gbest = Gnorm1_new;
        if (Gnorm1_new <= eps * Gnorm1_init) break;

        // inner coordinate descent on the quadratic model
        for (int i = lane; i < n; i += SV_THREADS) xTd[i] = 0.0;
        double QP_Gmax_old = 1e300;
        int QP_active = active, iter = 0;
        bool any_moved = false;
        while (iter < 1000) {
            // liblinear visits the active coordinates in a fresh random order every sweep (solve_l1r_lr); a fixed cyclic
            // order needs hundreds of times more sweeps on correlated columns (r01: 4.3 s against liblinear's 14 ms)
            if (lane == 0) {
                for (int jj = 0; jj + 1 < QP_active; jj++) {
                    rng ^= rng << 13; rng ^= rng >> 17; rng ^= rng << 5;
                    const int ii = jj + (int)(rng % (uint32_t)(QP_active - jj));
                    const int32_t tt = act[ii]; act[ii] = act[jj]; act[jj] = tt;
                }
            }
            double QP_Gmax_new = 0.0, QP_Gnorm1_new = 0.0;
            bool moved = false;
            for (int sidx = 0; sidx < QP_active; sidx++) {
                const int j = __builtin_amdgcn_readfirstlane(lane == 0 ? act[sidx] : 0);
                const float *col = XT + (size_t)j * n;
                const double H = FLD(&Hd[j]);
                const double wp = FLD(&wpd[j]);
                double G = 0.0;
                for (int i = lane; i < n; i += SV_THREADS) {
                    if (fold[i] == tf) continue;
                    const double x = (j < p) ? (double)col[i] : 1.0;
                    if (x != 0.0) G += x * D[i] * xTd[i];
                }
                G = psk_wave_sum_f64_dpp(G) + FLD(&Gr[j]) + (wp - FLD(&w[j])) * nu;
                const double pen = (PI || j < p) ? 1.0 : 0.0;
                const double Gp = G + pen, Gn = G - pen;
                double viol = 0.0;
                if (wp == 0.0) {
                    if (Gp < 0) viol = -Gp;
                    else if (Gn > 0) viol = Gn;
                    else if (Gp > QP_Gmax_old / l && Gn < -QP_Gmax_old / l) {  // inner shrinking
                        QP_active--;
                        if (lane == 0) { const int32_t t = act[sidx]; act[sidx] = act[QP_active]; act[QP_active] = t; }
                        sidx--;
                        continue;
                    }
                } else if (wp > 0) viol = fabs(Gp);
                else viol = fabs(Gn);
                if (viol > QP_Gmax_new) QP_Gmax_new = viol;
                QP_Gnorm1_new += viol;
                double z;
                if (Gp < H * wp) z = -Gp / H;
                else if (Gn > H * wp) z = -Gn / H;
                else z = -wp;
                // liblinear skips |z| < 1e-12; a coefficient that has drifted to ~1e-17 must still be allowed to land
                // on exactly 0, otherwise its +-1 subgradient term keeps the violation above the stopping threshold
                // forever (r01: 5 of 143 fits of a 256 x 138 problem spun to max_iter)
                if ((fabs(z) < zmin && !(z == -wp && wp != 0.0)) || z == 0.0) continue;
                z = fmin(fmax(z, -10.0), 10.0);
                moved = true;
                if (lane == 0) wpd[j] = wp + z;
                for (int i = lane; i < n; i += SV_THREADS) {
                    if (fold[i] == tf) continue;
                    const double x = (j < p) ? (double)col[i] : 1.0;
                    if (x != 0.0) xTd[i] += x * z;
                }
            }
            iter++;
            any_moved = any_moved || moved;
            // Every step of a whole sweep was below the 1e-12 that is skipped: no later sweep can move anything either.  With
            // count cells (x = 200: H ~ 4e4 D) that floor on a step leaves a gradient of ~1e-12 H, above the stop threshold of a
            // tight tolerance (r52: 64 x 1 and 65 x 3 counts at tol = 1e-12 swept 1000 times per Newton step until max_iter, and
            // 261 x 40 lay 1e-12 x the Hessian's condition number, 1e-8, from the optimum).  From the first such sweep on the
            // fit takes every step that is not zero; a sweep that moves nothing even so ends the descent.
            if (!moved && QP_active == active) {
                if (zmin > 0.0) { zmin = 0.0; continue; }
                break;
            }
            if (QP_Gnorm1_new <= inner_eps * Gnorm1_init) {
                if (QP_active == active) break;       // inner problem solved
                QP_active = active;                   // re-check the shrunk coordinates
                QP_Gmax_old = 1e300;
                continue;
            }
            QP_Gmax_old = QP_Gmax_new;
        }

        if (!any_moved) { newton++; break; }   // d = 0: no coordinate can move

        // line search along d = wpd - w
        double delta = 0.0, w_norm_new = 0.0;
        for (int j = 0; j < P1; j++) {
            const double wp = FLD(&wpd[j]);
            delta += FLD(&Gr[j]) * (wp - FLD(&w[j]));
            if (PI || j < p) w_norm_new += fabs(wp);
        }
        delta += (w_norm_new - w_norm);
        double negsum = 0.0;
        for (int i = lane; i < n; i += SV_THREADS)
            if (fold[i] != tf && ypm[i] < 0) negsum += C * xTd[i];
        negsum = psk_wave_sum_f64_dpp(negsum);
        bool accepted = false, floor_rebuild = false;
        for (int ls = 0; ls < 20; ls++) {
            double cs = 0.0;
            for (int i = lane; i < n; i += SV_THREADS) {
                if (fold[i] == tf) continue;
                const double ex = exp(xTd[i]);
                const double en = ewx[i] * ex;
                ewxn[i] = en;
                // exp(w.x) = inf (a count of 200 under a coefficient of 3.6: w.x > 709): the quotient is inf / inf; its limit is
                // exp(w.x) / (1 + exp(w.x)) of the point the step leaves.  (r52: 7 x 3 counts at C = 30, whose optimum has
                // w.x = 1018 on one row, rejected every step from w.x = 707 on and ended 9.7 % above the optimum at max_iter.)
                cs += C * (isinf(en) ? -log1p(1.0 / ewx[i]) : log((1.0 + en) / (ex + en)));
            }
            const double cond = w_norm_new - w_norm + negsum - sigma * delta + psk_wave_sum_f64_dpp(cs);
            // liblinear accepts when cond <= 0.  Close to the optimum the decrease the model predicts sinks below what the sum of
            // l logarithms can resolve in doubles (~C l 2^-52): the sign of cond is then noise, twenty halvings only make the
            // step smaller, and a fit run at a tolerance near that floor repeats the same rejected step until max_iter (r04:
            // fits at tol = 1e-12 either stopped after ~100 Newton steps or never).  A step whose cond is inside the noise is
            // taken whole -- near the optimum the quadratic model is the better judge -- and exp(w.x) is then rebuilt from w
            // (below: accepting such steps without it, the multiplicatively updated copy drifted over thousands of them and one
            // fit "converged" 26 % away); such steps in a row that gain nothing end the fit: it is where doubles can take it.  At the
            // tolerances the reference runs at |cond| is many orders above the noise and nothing changes.
            const bool in_noise = cond > 0.0 && cond <= 4.0 * 2.220446049250313e-16 * C * l;
            // (Counted are the steps in a row that did not bring the violation a tenth below its smallest so far, and five of
            // them end the fit: on count designs the steps inside the noise still converge -- r52: 261 x 40 counts at tol =
            // 1e-12 ended after three of them with the violation at 4e-7, falling, and a linear predictor 3 x its bound off.)
            // (once the fit has met the floor of its coordinate steps, zmin = 0, every accepted step that gains nothing counts)
            if (in_noise || (cond <= 0.0 && zmin == 0.0 && !progressed)) floor_steps = progressed ? 1 : floor_steps + 1;
            else if (cond <= 0.0) floor_steps = 0;
            if (cond <= 0.0 || in_noise) {
                w_norm = w_norm_new;
                for (int j = 0; j < P1; j++) { if (lane == 0) w[j] = wpd[j]; }
                double overflowed = 0.0;
                for (int i = lane; i < n; i += SV_THREADS) {
                    if (fold[i] == tf) continue;
                    const double en = ewxn[i];
                    const double tt = 1.0 / (1.0 + en);
                    ewx[i] = en; tau[i] = C * tt; D[i] = isinf(en) ? 0.0 : C * en * tt * tt;
                    if (isinf(en)) overflowed = 1.0;
                }
                accepted = true;
                // an inf forgets w.x: rebuilt from w below, exp(w.x) is inf exactly on the rows whose w.x is past 709
                floor_rebuild = in_noise || psk_wave_sum_f64_dpp(overflowed) > 0.0;
                break;
            }
            w_norm_new = 0.0;
            for (int j = 0; j < P1; j++) {
                const double v = 0.5 * (FLD(&w[j]) + FLD(&wpd[j]));
                if (lane == 0) wpd[j] = v;
                if (PI || j < p) w_norm_new += fabs(v);
            }
            delta *= 0.5;
            negsum *= 0.5;
            for (int i = lane; i < n; i += SV_THREADS) xTd[i] *= 0.5;
        }
        if (!accepted && zmin == 0.0 && !progressed) floor_steps++;
        if (!accepted || floor_rebuild) {
            // the step was rejected 20 times: fall back to the current w and, as liblinear does after "too many
            // line search steps", rebuild exp(w.x) from w -- the multiplicatively updated copy has drifted and
            // the gradient computed from it would reject every further step (r01: fits spinning to max_iter)
            for (int j = 0; j < P1; j++) { if (lane == 0) wpd[j] = w[j]; }
            for (int i = lane; i < n; i += SV_THREADS) xTd[i] = 0.0;
            for (int j = 0; j < P1; j++) {
                const double wj = FLD(&w[j]);
                if (wj == 0.0) continue;
                const float *col = XT + (size_t)j * n;
                for (int i = lane; i < n; i += SV_THREADS) xTd[i] += wj * (double)col[i];
            }
            for (int i = lane; i < n; i += SV_THREADS) {
                if (fold[i] == tf) continue;
                const double en = exp(xTd[i]);
                const double tt = 1.0 / (1.0 + en);
                ewx[i] = en; tau[i] = C * tt; D[i] = isinf(en) ? 0.0 : C * en * tt * tt;
            }
        }
        if (iter == 1) inner_eps *= 0.25;
        if (floor_steps >= 5) { newton++; break; }   // at the floor of what doubles resolve (see the line search)
        Gmax_old = Gmax_new;
    }
    for (int j = 0; j < p; j++) { if (lane == 0) coef[(size_t)fit * p + j] = w[j]; }
    if (lane == 0) { icpt[fit] = w[p]; iters[fit] = newton; }
}
#undef FLD

// EN (here and in lasso_bits_kernel): the elastic net of psk_enet_fit -- threshold alpha l1_ratio n, and
// beta = alpha (1 - l1_ratio) n in the step's divisor, in the dual norm max|X'R - beta w| and in the gap's
// 1/2 beta (1 + c^2) w'w.  A template parameter: the Lasso's instances (EN = false) compile to what they were.
template <bool EN>
__global__ __launch_bounds__(SV_THREADS) void lasso_kernel(const float *__restrict__ XT, const double *__restrict__ y,
                                                            const int32_t *__restrict__ fold, int n, int p,
                                                            const double *__restrict__ fit_param,
                                                            const int32_t *__restrict__ fit_fold, double tol, double l1_ratio, int max_iter,
                                                            double *__restrict__ coef, double *__restrict__ icpt,
                                                            int32_t *__restrict__ iters, double *__restrict__ work,
                                                            const int use_lds)
{
    extern __shared__ double sm[];
    const int fit = blockIdx.x, lane = threadIdx.x;
    const double alpha = fit_param[fit];
    const int tf = fit_fold[fit];
    double *w = coef + (size_t)fit * p;
    double *xm = work + (size_t)fit * (2 * (size_t)p + n);  // column means over the training rows
    double *nrm = xm + p;                                   // centred squared norms
    double *r = use_lds ? sm : nrm + p;                     // residual of the centred problem

    double sy = 0, cnt = 0;
    for (int i = lane; i < n; i += SV_THREADS)
        if (fold[i] != tf) { sy += y[i]; cnt += 1; }
    sy = psk_wave_sum_f64_dpp(sy);
    const double ntrain = psk_wave_sum_f64_dpp(cnt);
    const double ym = sy / ntrain;
    double yy = 0.0;   // y'y of the centred problem: scikit-learn's gap tolerance is tol y'y
    for (int i = lane; i < n; i += SV_THREADS) {
        const double d = (fold[i] != tf) ? (y[i] - ym) : 0.0;
        r[i] = d;
        yy += d * d;
    }
    yy = psk_wave_sum_f64_dpp(yy);
    const double an = EN ? (alpha * l1_ratio) * ntrain : alpha * ntrain, tol_s = tol * yy;
    const double beta = EN ? (alpha * (1.0 - l1_ratio)) * ntrain : 0.0;
    for (int j = 0; j < p; j++) {
        const float *col = XT + (size_t)j * n;
        double s1 = 0, s2 = 0;
        for (int i = lane; i < n; i += SV_THREADS)
            if (fold[i] != tf) { const double x = col[i]; s1 += x; s2 += x * x; }
        s1 = psk_wave_sum_f64_dpp(s1);
        s2 = psk_wave_sum_f64_dpp(s2);
        if (lane == 0) {
            const double m = s1 / ntrain;
            xm[j] = m;
            nrm[j] = s2 - ntrain * m * m;  // sum (x - m)^2
            w[j] = 0.0;
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    int sweep = 0;
    for (sweep = 0; sweep < max_iter; sweep++) {
        double dmax = 0.0, wmax = 0.0;
        for (int j = 0; j < p; j++) {
            const double nj = lane0_load(&nrm[j], lane);
            if (!(nj > 1e-12)) continue;
            const float *col = XT + (size_t)j * n;
            const double m = lane0_load(&xm[j], lane), wj = lane0_load(&w[j], lane);
            double s = 0.0;
            for (int i = lane; i < n; i += SV_THREADS)
                if (fold[i] != tf) s += ((double)col[i] - m) * r[i];
            const double rho = psk_wave_sum_f64_dpp(s) + nj * wj;
            const double mag = fabs(rho) - an;
            const double nw = (mag > 0.0) ? ((rho > 0 ? mag : -mag) / (EN ? nj + beta : nj)) : 0.0;
            const double dd = nw - wj;
            if (dd != 0.0) {
                for (int i = lane; i < n; i += SV_THREADS)
                    if (fold[i] != tf) r[i] -= dd * ((double)col[i] - m);
                if (lane == 0) w[j] = nw;
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
                __builtin_amdgcn_wave_barrier();
            }
            if (fabs(dd) > dmax) dmax = fabs(dd);
            if (fabs(nw) > wmax) wmax = fabs(nw);
        }
        // scikit-learn's stop (enet_coordinate_descent): after a sweep whose largest step is below tol x the largest
        // coefficient -- or the last sweep allowed -- the duality gap is evaluated and the descent ends when gap < tol y'y
        if (wmax == 0.0 || dmax / wmax < tol || sweep == max_iter - 1) {
            double dual = 0.0, l1 = 0.0, ww = 0.0;
            for (int j = 0; j < p; j++) {
                const float *col = XT + (size_t)j * n;
                const double m = lane0_load(&xm[j], lane);
                double s = 0.0;
                for (int i = lane; i < n; i += SV_THREADS)
                    if (fold[i] != tf) s += ((double)col[i] - m) * r[i];
                s = psk_wave_sum_f64_dpp(s);
                const double wj = lane0_load(&w[j], lane);
                if constexpr (EN) {
                    dual = fmax(dual, fabs(s - beta * wj));
                    ww += wj * wj;
                } else dual = fmax(dual, fabs(s));
                l1 += fabs(wj);
            }
            double rr = 0.0, ry = 0.0;
            for (int i = lane; i < n; i += SV_THREADS)
                if (fold[i] != tf) { rr += r[i] * r[i]; ry += r[i] * (y[i] - ym); }
            rr = psk_wave_sum_f64_dpp(rr);
            ry = psk_wave_sum_f64_dpp(ry);
            double cst = 1.0, gap;
            if (dual > an) { cst = an / dual; gap = 0.5 * (rr + rr * (cst * cst)); }
            else gap = rr;
            if constexpr (EN) gap += (an * l1 - cst * ry) + ((0.5 * beta) * (1.0 + cst * cst)) * ww;
            else gap += an * l1 - cst * ry;
            if (gap < tol_s) { sweep++; break; }
        }
    }
    double acc = 0.0;
    for (int j = 0; j < p; j++) acc += lane0_load(&xm[j], lane) * lane0_load(&w[j], lane);
    if (lane == 0) { icpt[fit] = ym - acc; iters[fit] = sweep; }
}

// Lasso on a 0/1 design (presence / absence: the default), four waves per fit, the samples in registers -- the layout and
// the EXEC-masked sums of cd_coop.  With x in {0, 1} the coordinate step of the kernel above needs no pass over all the
// samples: the residual is kept as r_i = r'_i + c (c: one scalar for the -dd * mean terms every training sample gets), so
//   sum (x - m) r  =  (S1 + c cnt) - m (R + c n),   S1 = sum of r' over the samples that have the k-mer (a masked sum),
//   R = sum of r' over the training samples (kept up to date),  cnt = their number with the k-mer,
// and the update is r' -= dd on those samples (a masked add), c += dd m, R -= dd cnt.  Same cyclic order, same soft
// threshold, same stop as lasso_kernel; column means and norms from the counts (x^2 = x).  The float kernel read a
// column of n floats from L2 per coordinate (~2.6 us at 1,024 samples); here it is one transposed word per lane, asked
// for a step ahead.  LDS: w | mean | norm | count, p doubles each.
template <int WM, bool EN>
__global__ __launch_bounds__(SV_COOP_THREADS) void lasso_bits_kernel(const uint64_t *__restrict__ colT, const double *__restrict__ y,
                                                                      const int32_t *__restrict__ fold, int n, int p, int W,
                                                                      const double *__restrict__ fit_param,
                                                                      const int32_t *__restrict__ fit_fold, double tol, double l1_ratio, int max_iter,
                                                                      double *__restrict__ coef, double *__restrict__ icpt,
                                                                      int32_t *__restrict__ iters)
{
    constexpr int WQ = WM / SV_COOP_WAVES;
    extern __shared__ double sm[];
    __shared__ double s_part[2][SV_COOP_WAVES];
    __shared__ double s_tot[2][SV_COOP_WAVES];
    double *w = sm, *mean = sm + p, *nrm = sm + 2 * (size_t)p, *cntd = sm + 3 * (size_t)p;
    uint32_t *cpart = reinterpret_cast<uint32_t *>(sm + 4 * (size_t)p);   // [wave][p] counts of this wave's samples
    const int fit = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6, t0 = wave * WQ;
    const double alpha = fit_param[fit];
    const int tf = fit_fold[fit];
    // this wave's training samples and their y
    double R[WQ], Yc[WQ];
    uint64_t tmask = 0;
    double sy = 0.0, cn = 0.0;
#pragma unroll
    for (int q = 0; q < WQ; q++) {
        const int t = t0 + q, i = t * 64 + lane;
        const bool tr = t < W && i < n && fold[i] != tf;
        R[q] = tr ? y[i] : 0.0;
        if (tr) { tmask |= 1ull << t; sy += R[q]; cn += 1.0; }
    }
    sy = psk_wave_sum_f64_dpp(sy);
    cn = psk_wave_sum_f64_dpp(cn);
    if (lane == 0) { s_part[0][wave] = sy; s_tot[0][wave] = cn; }
    // this wave's share of every column's count
    for (int j = 0; j < p; j++) {
        const uint64_t x = colT[(size_t)j * 64 + lane] & tmask;
        uint32_t c = (uint32_t)__popcll(x);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) c += __shfl_xor(c, d, 64);
        if (lane == 0) cpart[(size_t)wave * p + j] = c;
    }
    __syncthreads();
    double ysum = s_part[0][0], ntrain = s_tot[0][0];
#pragma unroll
    for (int v = 1; v < SV_COOP_WAVES; v++) { ysum += s_part[0][v]; ntrain += s_tot[0][v]; }
    const double ym = ysum / ntrain;
    double yyw = 0.0;
#pragma unroll
    for (int q = 0; q < WQ; q++) {
        if ((tmask >> (t0 + q)) & 1) R[q] -= ym;
        Yc[q] = R[q];            // the centred y of the training samples (0 elsewhere): R'y of the duality gap
        yyw += R[q] * R[q];
    }
    yyw = psk_wave_sum_f64_dpp(yyw);
    if (lane == 0) s_tot[1][wave] = yyw;
    for (int j = threadIdx.x; j < p; j += SV_COOP_THREADS) {
        uint32_t c = 0;
#pragma unroll
        for (int v = 0; v < SV_COOP_WAVES; v++) c += cpart[(size_t)v * p + j];
        const double s1 = (double)c, m = s1 / ntrain;
        cntd[j] = s1;
        mean[j] = m;
        nrm[j] = s1 - ntrain * m * m;   // sum (x - m)^2 with x^2 = x
        w[j] = 0.0;
    }
    // R' = sum of r' over the training samples: every wave sums its own, all of them add the four parts
    double Rw = 0.0;
#pragma unroll
    for (int q = 0; q < WQ; q++) Rw += R[q];
    Rw = psk_wave_sum_f64_dpp(Rw);
    if (lane == 0) s_part[1][wave] = Rw;
    __syncthreads();
    double Rp = s_part[1][0], yy = s_tot[1][0];
#pragma unroll
    for (int v = 1; v < SV_COOP_WAVES; v++) { Rp += s_part[1][v]; yy += s_tot[1][v]; }
    __syncthreads();
    const double an = EN ? (alpha * l1_ratio) * ntrain : alpha * ntrain, tol_s = tol * yy;
    const double beta = EN ? (alpha * (1.0 - l1_ratio)) * ntrain : 0.0;
    double c = 0.0;
    int sweep = 0, visit = 0;
    auto col_t = [&](int j) { return (colT[(size_t)j * 64 + lane] & tmask) >> t0; };
    for (sweep = 0; sweep < max_iter; sweep++) {
        double dmax = 0.0, wmax = 0.0;
        uint64_t m_next = p > 0 ? col_t(0) : 0ull;
        for (int j = 0; j < p; j++) {
            const uint64_t x = m_next;
            if (j + 1 < p) m_next = col_t(j + 1);
            const double nj = nrm[j];
            if (!(nj > 1e-12)) continue;
            const double mj = mean[j], wj = w[j], cj = cntd[j];
            uint64_t M[WQ];
#pragma unroll
            for (int q = 0; q < WQ; q++) M[q] = __ballot((x >> q) & 1ull);
            double S = 0.0;
            if (WQ == 16) { masked_sum8(S, M, R); masked_sum8(S, M + (WQ == 16 ? 8 : 0), R + (WQ == 16 ? 8 : 0)); }
            else if (WQ == 8) masked_sum8(S, M, R);
            else masked_sum4(S, M, R);
            S = psk_wave_sum_f64_dpp(S);
            const int slot = visit & 1;
            visit++;
            if (lane == 0) s_part[slot][wave] = S;
            __syncthreads();
            double S1 = s_part[slot][0];
#pragma unroll
            for (int v = 1; v < SV_COOP_WAVES; v++) S1 += s_part[slot][v];
            const double rho = ((S1 + c * cj) - mj * (Rp + c * ntrain)) + nj * wj;
            const double mag = fabs(rho) - an;
            const double nw = (mag > 0.0) ? ((rho > 0 ? mag : -mag) / (EN ? nj + beta : nj)) : 0.0;
            const double dd = nw - wj;
            if (dd != 0.0) {
                const double nd = -dd;
                if (WQ == 16) { masked_add8(R, M, nd); masked_add8(R + (WQ == 16 ? 8 : 0), M + (WQ == 16 ? 8 : 0), nd); }
                else if (WQ == 8) masked_add8(R, M, nd);
                else masked_add4(R, M, nd);
                c += dd * mj;
                Rp -= dd * cj;
                if (threadIdx.x == 0) w[j] = nw;   // read again a sweep later, many barriers from here
            }
            if (fabs(dd) > dmax) dmax = fabs(dd);
            if (fabs(nw) > wmax) wmax = fabs(nw);
        }
        __syncthreads();   // w of this sweep is in place for the next one (and for the end)
        // scikit-learn's stop (see lasso_kernel): the duality gap, when it would evaluate it.  X'R of every column is one
        // more pass of masked sums (no steps), R'R and R'y come from the registers (r = r' + c on the training samples)
        if (wmax == 0.0 || dmax / wmax < tol || sweep == max_iter - 1) {
            double dual = 0.0, l1 = 0.0, ww = 0.0;
            uint64_t mg_next = p > 0 ? col_t(0) : 0ull;
            for (int j = 0; j < p; j++) {
                const uint64_t x = mg_next;
                if (j + 1 < p) mg_next = col_t(j + 1);
                uint64_t M[WQ];
#pragma unroll
                for (int q = 0; q < WQ; q++) M[q] = __ballot((x >> q) & 1ull);
                double S = 0.0;
                if (WQ == 16) { masked_sum8(S, M, R); masked_sum8(S, M + (WQ == 16 ? 8 : 0), R + (WQ == 16 ? 8 : 0)); }
                else if (WQ == 8) masked_sum8(S, M, R);
                else masked_sum4(S, M, R);
                S = psk_wave_sum_f64_dpp(S);
                const int slot = visit & 1;
                visit++;
                if (lane == 0) s_part[slot][wave] = S;
                __syncthreads();
                double S1 = s_part[slot][0];
#pragma unroll
                for (int v = 1; v < SV_COOP_WAVES; v++) S1 += s_part[slot][v];
                const double xr = (S1 + c * cntd[j]) - mean[j] * (Rp + c * ntrain);
                if constexpr (EN) {
                    dual = fmax(dual, fabs(xr - beta * w[j]));
                    ww += w[j] * w[j];
                } else dual = fmax(dual, fabs(xr));
                l1 += fabs(w[j]);
            }
            double rr = 0.0, ry = 0.0;
#pragma unroll
            for (int q = 0; q < WQ; q++)
                if ((tmask >> (t0 + q)) & 1) { const double rv = R[q] + c; rr += rv * rv; ry += rv * Yc[q]; }
            rr = psk_wave_sum_f64_dpp(rr);
            ry = psk_wave_sum_f64_dpp(ry);
            __syncthreads();
            if (lane == 0) { s_part[0][wave] = rr; s_part[1][wave] = ry; }
            __syncthreads();
            rr = (s_part[0][0] + s_part[0][1]) + (s_part[0][2] + s_part[0][3]);
            ry = (s_part[1][0] + s_part[1][1]) + (s_part[1][2] + s_part[1][3]);
            __syncthreads();
            double cst = 1.0, gap;
            if (dual > an) { cst = an / dual; gap = 0.5 * (rr + rr * (cst * cst)); }
            else gap = rr;
            if constexpr (EN) gap += (an * l1 - cst * ry) + ((0.5 * beta) * (1.0 + cst * cst)) * ww;
            else gap += an * l1 - cst * ry;
            if (gap < tol_s) { sweep++; break; }
        }
    }
    double acc = 0.0;
    for (int j = threadIdx.x; j < p; j += SV_COOP_THREADS) {
        coef[(size_t)fit * p + j] = w[j];
        acc += mean[j] * w[j];
    }
    acc = psk_wave_sum_f64_dpp(acc);
    if (lane == 0) s_tot[1][wave] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double a = s_tot[1][0];
#pragma unroll
        for (int v = 1; v < SV_COOP_WAVES; v++) a += s_tot[1][v];
        icpt[fit] = ym - a;
        iters[fit] = sweep;
    }
}

// the distinct held-out folds of a call in order of first use; of_fit[j]: index of fit j's fold among them
std::vector<int32_t> distinct_folds(const int32_t *fit_fold, int n_fits, std::vector<int32_t> &of_fit)
{
    std::vector<int32_t> ids;
    of_fit.resize(n_fits);
    for (int j = 0; j < n_fits; j++) {
        size_t q = 0;
        while (q < ids.size() && ids[q] != fit_fold[j]) q++;
        if (q == ids.size()) ids.push_back(fit_fold[j]);
        of_fit[j] = (int32_t)q;
    }
    return ids;
}

// the covariance form (solver_lasso.hip): fits of one fold share its co-occurrence counts
// the penalty of a call: the Lasso (psk_lasso_fit), or the elastic net with its mixing parameter (psk_enet_fit)
struct LassoPenalty {
    bool enet;
    double l1_ratio;
};

int lasso_cov_fit(psk_ctx *ctx, const FitArgs &a, const double *y, const std::vector<int32_t> &fold_ids,
                  const std::vector<int32_t> &fidx, double tol, int max_iter, LassoPenalty pen)
{
    const int n = a.n, p = a.p, n_fits = a.n_fits, W = (n + 63) / 64, PP = 64 * ((p + 63) / 64), F = (int)fold_ids.size();
    const std::vector<uint64_t> bits = pack_sample_bits(a.X, n, p, W, PP, false);
    std::vector<uint64_t> tmask((size_t)F * W, 0);
    std::vector<double> yc((size_t)F * n, 0.0), fstat((size_t)F * 4, 0.0);
    for (int f = 0; f < F; f++) {
        double sy = 0.0, cnt = 0.0, yy = 0.0;
        for (int i = 0; i < n; i++)
            if (a.fold[i] != fold_ids[f]) { sy += y[i]; cnt += 1.0; tmask[(size_t)f * W + (i >> 6)] |= 1ull << (i & 63); }
        if (cnt < 1.0) return psk_fail(ctx, PSK_EINVAL, "fold %d leaves no training sample", fold_ids[f]);
        const double ym = sy / cnt;
        for (int i = 0; i < n; i++)
            if (a.fold[i] != fold_ids[f]) { const double d = y[i] - ym; yc[(size_t)f * n + i] = d; yy += d * d; }
        fstat[4 * f] = ym; fstat[4 * f + 1] = yy; fstat[4 * f + 2] = cnt;
    }
    // Workgroups go round the eight XCDs (workgroup b runs on XCD b % 8), each with its own 4-MB L2: the fits are
    // ordered by fold and XCD x takes a contiguous stretch of that order, so that the fits sharing an L2 read the
    // same one or two count matrices (1.6 MB each at 907 columns)
    std::vector<int32_t> order(n_fits);
    for (int j = 0; j < n_fits; j++) order[j] = j;
    std::stable_sort(order.begin(), order.end(), [&](int32_t u, int32_t v) { return fidx[u] < fidx[v]; });
    const int G = (n_fits + 7) / 8, n_blocks = 8 * G;
    std::vector<int32_t> block_fit(n_blocks, -1);
    for (int bq = 0; bq < n_blocks; bq++) {
        const int sidx = (bq % 8) * G + bq / 8;
        if (sidx < n_fits) block_fit[bq] = order[sidx];
    }
    FitIO io;
    FitArr<uint64_t> d_bits, d_tmask;
    FitArr<double> d_yc, d_fstat, d_Dg, d_q0;
    FitArr<uint16_t> d_C;
    FitArr<int32_t> d_bf, d_fidx;
    PSK_TRY(io.upload(ctx, a, false));   // the kernels read tmask and fidx, not the folds
    PSK_HIP(ctx, d_bits.upload(bits, ctx->stream));
    PSK_HIP(ctx, d_tmask.upload(tmask, ctx->stream));
    PSK_HIP(ctx, d_yc.upload(yc, ctx->stream));
    PSK_HIP(ctx, d_fstat.upload(fstat, ctx->stream));
    PSK_HIP(ctx, d_C.alloc((size_t)F * PP * PP));
    PSK_HIP(ctx, d_Dg.alloc((size_t)F * (PP / 64) * 4096));
    PSK_HIP(ctx, d_q0.alloc((size_t)F * PP));
    PSK_HIP(ctx, d_bf.upload(block_fit, ctx->stream));
    PSK_HIP(ctx, d_fidx.upload(fidx, ctx->stream));
    psk_lasso_cov_args A;
    A.bits = d_bits; A.tmask = d_tmask; A.yc = d_yc; A.fstat = d_fstat; A.C = d_C; A.Dg = d_Dg; A.q0 = d_q0;
    A.block_fit = d_bf; A.fit_param = io.fit_param; A.fit_fidx = d_fidx;
    A.n = n; A.p = p; A.PP = PP; A.W = W; A.n_folds = F; A.n_blocks = n_blocks; A.max_iter = max_iter; A.tol = tol;
    A.enet = pen.enet; A.l1_ratio = pen.l1_ratio;
    A.coef = io.coef; A.icpt = io.icpt; A.gaps = nullptr; A.iters = io.iters; A.stream = ctx->stream;
    PSK_HIP(ctx, psk_lasso_cov_launch(A));
    return io.download(ctx, a);
}

// the four-wave kernel on the bit-packed samples; `lds`: its per-column state
int lasso_bits_fit(psk_ctx *ctx, const FitArgs &a, const double *y, size_t lds, double tol, int max_iter, LassoPenalty pen)
{
    const int n = a.n, p = a.p, W = (n + 63) / 64;
    const std::vector<uint64_t> bitsT = pack_lane_bits(a.X, n, p, false);
    FitIO io;
    FitArr<uint64_t> d_bitsT;
    FitArr<double> d_y;
    PSK_TRY(io.upload(ctx, a));
    PSK_HIP(ctx, d_bitsT.upload(bitsT, ctx->stream));
    PSK_HIP(ctx, d_y.upload(y, n, ctx->stream));
    auto kern = W <= 16 ? lasso_bits_kernel<16, false> : W <= 32 ? lasso_bits_kernel<32, false> : lasso_bits_kernel<64, false>;
    if (pen.enet) kern = W <= 16 ? lasso_bits_kernel<16, true> : W <= 32 ? lasso_bits_kernel<32, true> : lasso_bits_kernel<64, true>;
    if (lds > 64 * 1024)
        PSK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<a.n_fits, SV_COOP_THREADS, lds, ctx->stream>>>(d_bitsT, d_y, io.fold, n, p, W, io.fit_param, io.fit_fold, tol, pen.l1_ratio,
                                                          max_iter, io.coef, io.icpt, io.iters);
    return io.download(ctx, a);
}

int lasso_float_fit(psk_ctx *ctx, const FitArgs &a, const double *y, double tol, int max_iter, LassoPenalty pen)
{
    const int n = a.n, p = a.p;
    const std::vector<float> XT = transpose_f32(a.X, n, p, true);
    const int use_lds = n <= 2 * SV_LDS_N ? 1 : 0;   // one residual array: 8 KiB samples fit
    const size_t lds = use_lds ? (size_t)n * sizeof(double) : 0;
    FitIO io;
    FitArr<float> xt;
    FitArr<double> d_y, work;
    PSK_TRY(io.upload(ctx, a));
    PSK_HIP(ctx, xt.upload(XT, ctx->stream));
    PSK_HIP(ctx, d_y.upload(y, n, ctx->stream));
    PSK_HIP(ctx, work.alloc((size_t)a.n_fits * (2 * (size_t)p + n)));
    auto kern = pen.enet ? lasso_kernel<true> : lasso_kernel<false>;
    kern<<<a.n_fits, SV_THREADS, lds, ctx->stream>>>(xt, d_y, io.fold, n, p, io.fit_param, io.fit_fold, tol, pen.l1_ratio, max_iter, io.coef,
                                                     io.icpt, io.iters, work, use_lds);
    return io.download(ctx, a);
}

// psk_logreg_l1_fit (pen_icpt: liblinear's penalised intercept) and psk_logreg_l1_free_fit (the free one) after their
// arguments are checked: the same knobs, routes and placements, the kernels' PI instances apart
int logreg_l1_route(psk_ctx *ctx, const FitArgs &a, const int32_t *y01, double tol, int max_iter, bool pen_icpt)
{
    const float *X = a.X;
    const int n = a.n, p = a.p, n_fits = a.n_fits;
    // form knobs, validated before anything is allocated
    psk_l1_knobs k;
    int knob_cg_max = 16, knob_polish_from = 32;
    k.no_cd_regs = env_flag("PSK_NO_CD_REGS"); k.no_gram = env_flag("PSK_NO_GRAM"); k.no_gram_global = env_flag("PSK_NO_GRAM_GLOBAL");
    PSK_TRY(env_int(ctx, "PSK_GG_MIN_P1", 1, 1 << 20, &k.min_p1, &k.set_min_p1));
    PSK_TRY(env_choice(ctx, "PSK_FORCE_WMREG", {16, 32, 64}, &k.force_wmreg));   // (0: n picks the register form)
    PSK_TRY(env_int(ctx, "PSK_CG_MAX", 0, 256, &knob_cg_max));
    PSK_TRY(env_int(ctx, "PSK_POLISH_REPS", -4096, 4096, &k.polish_reps, &k.set_reps));
    PSK_TRY(env_int(ctx, "PSK_GG_POLISH_FROM", 1, 1000, &knob_polish_from));
    if (k.force_wmreg && k.force_wmreg * 64 < n)
        return psk_fail(ctx, PSK_EINVAL, "PSK_FORCE_WMREG=%d holds %d samples, the design has %d", k.force_wmreg, k.force_wmreg * 64, n);
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    // presence/absence design (every entry 0 or 1)?  -> bit-packed kernel, which keeps a column in one register per lane (64 words)
    const bool binary = n <= 4096 && design_is_binary(X, (size_t)n * p);
    const int W = (n + 63) / 64;
    const size_t n_state = binary ? (size_t)W * 64 : (size_t)n;
    const std::vector<int8_t> ypm = labels_pm1(y01, n);
    FitIO io;
    FitArr<int8_t> y;
    FitArr<double> work;
    FitArr<int32_t> iwork;
    PSK_TRY(io.upload(ctx, a));
    PSK_HIP(ctx, y.upload(ypm, ctx->stream));
    PSK_HIP(ctx, work.alloc((size_t)n_fits * 5 * ((size_t)(p + 1) + n_state)));   // per fit: five feature, five sample arrays
    PSK_HIP(ctx, iwork.alloc((size_t)n_fits * (p + 1)));
    if (binary) {
        const std::vector<uint64_t> bits = pack_sample_bits(X, n, p, W, p + 1, true);
        // the same columns transposed for the register form of the descent
        const std::vector<uint64_t> bitsT = k.no_cd_regs ? std::vector<uint64_t>() : pack_lane_bits(X, n, p, true);
        FitArr<uint64_t> d_bits, d_bitsT;
        FitArr<float> ggq;
        PSK_HIP(ctx, d_bits.upload(bits, ctx->stream));
        if (!bitsT.empty()) PSK_HIP(ctx, d_bitsT.upload(bitsT, ctx->stream));
        psk_l1_placement P = psk_l1_gg_wanted(n, p, W, n_fits, k, SV_COOP_WAVES);
        // (a device too full for the Gram matrices keeps the array form: slower, the same optimum)
        if (P.gg_sl && ggq.alloc((size_t)n_fits * P.gg_stride) != hipSuccess) { (void)hipGetLastError(); P = psk_l1_placement(); }
        P = psk_l1_place(p, W, k, P);
        psk_l1_bits_launch L;
        L.bits = d_bits; L.bitsT = d_bitsT; L.ypm = y;
        L.fold = io.fold; L.fit_fold = io.fit_fold; L.fit_param = io.fit_param;
        L.n = n; L.p = p; L.W = W; L.n_fits = n_fits; L.max_iter = max_iter; L.tol = tol;
        L.coef = io.coef; L.icpt = io.icpt; L.work = work; L.iters = io.iters; L.iwork = iwork;
        L.f_lds = P.f_lds; L.s_lds = P.s_lds; L.c_lds = P.c_lds; L.q_doubles = P.q_doubles;
        // CG steps per polish (the Gram-global form uses a quarter of them, at least 4, while steps are cut short early)
        L.cg_max = knob_cg_max;
        L.polish_reps = P.polish_reps;
        L.gg_sl = P.gg_sl; L.gg_q = ggq; L.gg_stride = P.gg_stride;
        L.gg_polish_from = knob_polish_from;   // first polish of a descent after this many sweeps
        L.wmreg = P.wmreg; L.all_lds = P.all_lds; L.lds_bytes = P.lds_bytes; L.stream = ctx->stream;
        L.pen_icpt = pen_icpt ? 1 : 0;
        // two kernels, compiled apart (solver_l1_bits.h): the Gram matrix in global memory, or the LDS Gram block / array forms
        PSK_HIP(ctx, P.gg_sl ? psk_l1_bits_launch_gg(L) : psk_l1_bits_launch_gram(L));
        return io.download(ctx, a);   // (synchronises: `bits` and `bitsT` outlive their copies)
    }
    // placement of the per-fit state: everything in LDS when it fits the 160 KiB of a CU, else the sample
    // arrays only, else global scratch
    const size_t fbytes = psk_l1_feature_bytes(p), sbytes = 5 * n_state * 8;
    int f_lds = 0, s_lds = 0;
    if (fbytes + sbytes <= PSK_L1_LDS_MAX) f_lds = s_lds = 1;
    else if (sbytes <= PSK_L1_LDS_MAX) s_lds = 1;
    else if (fbytes <= PSK_L1_LDS_MAX) f_lds = 1;
    const size_t lds = (f_lds ? fbytes : 0) + (s_lds ? sbytes : 0);
    const std::vector<float> XT = transpose_f32(X, n, p, true);
    FitArr<float> xt;
    PSK_HIP(ctx, xt.upload(XT, ctx->stream));
    auto kern = pen_icpt ? logreg_newglmnet_kernel<true> : logreg_newglmnet_kernel<false>;
    if (lds > 64 * 1024)
        PSK_HIP(ctx, hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    kern<<<n_fits, SV_THREADS, lds, ctx->stream>>>(xt, y, io.fold, n, p, io.fit_param, io.fit_fold, tol, max_iter, io.coef, io.icpt, io.iters,
                                                   work, iwork, f_lds, s_lds);
    return io.download(ctx, a);
}

}  // namespace

extern "C" int psk_logreg_l1_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                                 const double *fit_param, const int32_t *fit_fold, int n_fits, double tol, int max_iter,
                                 double *coef_out, double *icpt_out, int32_t *iters_out)
{
    const FitArgs a = {X, n, p, fold, fit_param, fit_fold, n_fits, coef_out, icpt_out, iters_out};
    PSK_TRY(check_fit_args(ctx, a, y01));
    return logreg_l1_route(ctx, a, y01, tol, max_iter, true);
}

extern "C" int psk_logreg_l1_free_fit(psk_ctx *ctx, const float *X, const int32_t *y01, int n, int p, const int32_t *fold,
                                      const double *fit_param, const int32_t *fit_fold, int n_fits, double tol, int max_iter,
                                      double *coef_out, double *icpt_out, int32_t *iters_out)
{
    const FitArgs a = {X, n, p, fold, fit_param, fit_fold, n_fits, coef_out, icpt_out, iters_out};
    PSK_TRY(check_fit_args(ctx, a, y01));
    // a free intercept runs off to infinity on a training set of one class: there is no minimiser
    for (int f = 0; f < n_fits; f++) {
        int c0 = 0, c1 = 0;
        for (int i = 0; i < n; i++)
            if (fold[i] != fit_fold[f]) { if (y01[i]) c1++; else c0++; }
        if (!c0 || !c1)
            return psk_fail(ctx, PSK_EINVAL, "psk_logreg_l1_free_fit: fit %d trains on one class only (%d of class 0, %d of class 1)", f, c0, c1);
    }
    return logreg_l1_route(ctx, a, y01, tol, max_iter, false);
}

namespace {

// the route of a Lasso or elastic-net call, after its arguments are checked
int lasso_route(psk_ctx *ctx, const FitArgs &a, const double *y, double tol, int max_iter, LassoPenalty pen)
{
    const int n = a.n, p = a.p;
    PSK_HIP(ctx, hipSetDevice(ctx->device));
    // presence/absence design (every entry 0 or 1): the covariance form up to 1,024 columns and 2 GiB of count matrices, else
    // the four-wave kernel on the bit-packed samples while its per-column state fits in LDS; else the float kernel.
    // PSK_NO_LASSO_COV / PSK_NO_LASSO_BITS for A/B runs
    const bool binary = n <= 4096 && !env_flag("PSK_NO_LASSO_BITS") && design_is_binary(a.X, (size_t)n * p);
    if (binary && p <= 1024 && !env_flag("PSK_NO_LASSO_COV")) {
        std::vector<int32_t> fidx;
        const std::vector<int32_t> fold_ids = distinct_folds(a.fit_fold, a.n_fits, fidx);
        const size_t PP = 64 * (((size_t)p + 63) / 64);
        if (fold_ids.size() * PP * PP * 2 <= ((size_t)2 << 30)) return lasso_cov_fit(ctx, a, y, fold_ids, fidx, tol, max_iter, pen);
    }
    const size_t lds_bits = (size_t)p * (4 * 8 + SV_COOP_WAVES * 4);
    if (binary && lds_bits <= 150 * 1024) return lasso_bits_fit(ctx, a, y, lds_bits, tol, max_iter, pen);
    return lasso_float_fit(ctx, a, y, tol, max_iter, pen);
}

}  // namespace

extern "C" int psk_lasso_fit(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold,
                             const double *fit_param, const int32_t *fit_fold, int n_fits, double tol, int max_iter,
                             double *coef_out, double *icpt_out, int32_t *iters_out)
{
    const FitArgs a = {X, n, p, fold, fit_param, fit_fold, n_fits, coef_out, icpt_out, iters_out};
    PSK_TRY(check_fit_args(ctx, a, y));
    return lasso_route(ctx, a, y, tol, max_iter, LassoPenalty{false, 1.0});
}

extern "C" int psk_enet_fit(psk_ctx *ctx, const float *X, const double *y, int n, int p, const int32_t *fold,
                            const double *fit_alpha, const int32_t *fit_fold, int n_fits, double l1_ratio, double tol,
                            int max_iter, double *coef_out, double *icpt_out, int32_t *iters_out)
{
    const FitArgs a = {X, n, p, fold, fit_alpha, fit_fold, n_fits, coef_out, icpt_out, iters_out};
    PSK_TRY(check_fit_args(ctx, a, y));
    if (!(l1_ratio >= 0.0 && l1_ratio <= 1.0))   // (a nan fails both comparisons)
        return psk_fail(ctx, PSK_EINVAL, "l1_ratio must lie in [0, 1], got %g", l1_ratio);
    return lasso_route(ctx, a, y, tol, max_iter, LassoPenalty{true, l1_ratio});
}
