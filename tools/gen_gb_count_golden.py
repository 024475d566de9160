#!/usr/bin/env python3
"""Records tests/golden/gb_count_kat.npz from scikit-learn's GradientBoostingRegressor / GradientBoostingClassifier fitted on
COUNT designs (the file notes the version; 1.7.2 is the contract of `-bc XGBC` / `-reg XGBR` under `--real_counts`, DESIGN.md
section 5).  The count twin of tools/gen_gb_golden.py: the same cases, the same record per case, the same bound.

Designs: synthetic k-mer count matrices of 96 samples x 40 columns with a 3-fold vector; three with a continuous target (squared
error, 8 genes), three with a 0/1 target (log loss, 4 genes).  A gene's copy number is present * choice([1, 1, 2, 3, 5]) per
sample; a column is its gene's copy number times choice([1, 1, 2]) (a k-mer that occurs once or twice in the gene); every eighth
column is binarised.  The target depends on a copy number, on a threshold (copies >= 2) and on a presence, so scikit-learn splits
at thresholds other than 0.5.  Per design four cases of 30 stages at depth 3 -- all samples in bag, and each fold held out; the
first continuous design also gives a depth-4 case and the first 0/1 design a depth-1 case, of 10 stages on all samples.  Per case,
from scikit-learn fitted on the in-bag rows of the float32 count matrix with random_state 0: staged_predict /
staged_decision_function, predict and predict_proba of those rows, the initial raw value, train_score_ and the set of split
thresholds it used; d_ref, the largest absolute difference of the staged values between fits with random_state 0, 1 and 2; and
bound = 8 * max(d_ref, 2^-52 * max|F|).  Nothing here is measured against the code under test.

A design is kept only when it is DECISIVE in every one of its cases (tests/gb_count_restated.py's diagnostic on the restatement of
the contract): at every split the winning proxy P1 and the best proxy P2 of a threshold plane with a different partition of the
node's in-bag samples satisfy (P1 - P2) / P1 >= 1e-9, and every node whose targets differ has impurity >= 1e-12.  The generator
walks seeds 0 .. 63 and keeps the first three of either kind; the file records the seeds kept and skipped.
usage: tools/gen_gb_count_golden.py"""
import os
import sys

import numpy as np
import sklearn
from sklearn.ensemble import GradientBoostingClassifier, GradientBoostingRegressor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import gb_count_restated as C  # noqa: E402
import gb_restated as R  # noqa: E402

N, P, FOLDS, STAGES, DEPTH, RATE = 96, 40, 3, 30, 3, 0.1
MARGIN, MIN_IMPURITY, MAX_SEED = 1e-9, 1e-12, 64
GENES = {0: 8, 1: 4}     # distinct presence patterns by loss, as in tools/gen_gb_golden.py


def design(seed, loss):
    G = GENES[loss]
    rng = np.random.default_rng(5000 + 1000 * loss + seed)
    present = (rng.random((N, G)) < rng.uniform(.3, .7, G)).astype(np.int64)
    copies = present * rng.choice([1, 1, 2, 3, 5], (N, G))
    of = np.concatenate([np.arange(G), rng.integers(0, G, P - G)])
    rng.shuffle(of)
    X = copies[:, of] * rng.choice([1, 1, 2], P)[None, :]
    X[:, 7::8] = X[:, 7::8] > 0
    a, b, c = rng.choice(G, 3, replace=False)
    if loss == 0:
        y = 0.8 * copies[:, a] - 1.5 * (copies[:, b] >= 2) + 1.0 * present[:, c] + 0.3 * rng.normal(0.0, 1.0, N)
    else:
        z = 0.8 * copies[:, a] - 2.0 * (copies[:, b] >= 2) + 1.5 * present[:, c] - 0.5
        y = (rng.random(N) < 1.0 / (1.0 + np.exp(-z))).astype(np.float64)
    return X.astype(np.float32), y, (rng.permutation(N) % FOLDS).astype(np.int32)


def case_list(first, loss):
    """(held-out fold, stages, depth); the first design with a continuous target adds the depth-4 case, the first with a 0/1
    target the depth-1 case."""
    cases = [(ff, STAGES, DEPTH) for ff in (-1, 0, 1, 2)]
    return cases + [(-1, 10, 1 if loss else 4)] if first else cases


def sk_case(X, y, in_bag, loss, stages, depth):
    Xt, yt = X[in_bag].astype(np.float32), y[in_bag]
    staged = []
    for rs in (0, 1, 2):
        if loss == 0:
            m = GradientBoostingRegressor(n_estimators=stages, max_depth=depth, random_state=rs).fit(Xt, yt)
            staged.append(np.array(list(m.staged_predict(Xt))))
        else:
            m = GradientBoostingClassifier(n_estimators=stages, max_depth=depth, random_state=rs).fit(Xt, yt.astype(np.int64))
            staged.append(np.array(list(m.staged_decision_function(Xt))).reshape(stages, -1))
        if rs == 0:
            first = m
    d_ref = max(float(np.abs(staged[0] - s).max()) for s in staged[1:])
    init = float(first._raw_predict_init(Xt[:1])[0, 0])
    used = np.unique(np.concatenate([e.tree_.threshold[e.tree_.children_left != -1] for e in first.estimators_[:, 0]]))
    rec = dict(staged=staged[0], predict=first.predict(Xt), init=init, train_score=first.train_score_.copy(), d_ref=d_ref,
               bound=8.0 * max(d_ref, 2.0 ** -52 * float(np.abs(staged[0]).max())), thresholds=used)
    rec["proba"] = first.predict_proba(Xt) if loss == 1 else np.zeros((0, 2))
    return rec


def decisive(X, y, fold, loss, cases):
    for ff, stages, depth in cases:
        in_bag = fold != ff
        f = C.fit_one(X, y, in_bag, loss, stages, RATE, depth, R.init_raw(y, in_bag, loss), diagnose=True)
        if not (f["margin"] >= MARGIN and f["min_impurity"] >= MIN_IMPURITY):
            return False
    return True


def main():
    out = {"sklearn_version": np.array(sklearn.__version__), "learning_rate": np.array(RATE)}
    case_design, case_fit_fold, case_loss, case_stages, case_depth = [], [], [], [], []
    k = 0
    for loss in (0, 1):
        kept, skipped = [], []
        for seed in range(MAX_SEED):
            X, y, fold = design(seed, loss)
            cases = case_list(not kept, loss)
            if not decisive(X, y, fold, loss, cases):
                skipped.append(seed)
                continue
            d = len(kept) + 3 * loss
            out["X_%d" % d], out["y_%d" % d], out["fold_%d" % d] = X, y, fold
            for ff, stages, depth in cases:
                rec = sk_case(X, y, fold != ff, loss, stages, depth)
                for name, v in rec.items():
                    out["%s_%d" % (name, k)] = np.asarray(v)
                case_design.append(d), case_fit_fold.append(ff), case_loss.append(loss), case_stages.append(stages), case_depth.append(depth)
                print("case %2d design %d loss %d fit_fold %2d stages %2d depth %d  d_ref %.3g  bound %.3g  thresholds %s" %
                      (k, d, loss, ff, stages, depth, rec["d_ref"], rec["bound"], " ".join("%g" % t for t in rec["thresholds"])))
                k += 1
            kept.append(seed)
            if len(kept) == 3:
                break
        assert len(kept) == 3, "fewer than three decisive designs of loss %d within %d seeds" % (loss, MAX_SEED)
        out["seeds_kept_%d" % loss], out["seeds_skipped_%d" % loss] = np.array(kept), np.array(skipped, dtype=np.int64)
        print("loss %d: seeds kept %s, skipped %s" % (loss, kept, skipped))
    out.update(case_design=np.array(case_design), case_fit_fold=np.array(case_fit_fold), case_loss=np.array(case_loss),
               case_stages=np.array(case_stages), case_depth=np.array(case_depth))
    path = os.path.join(ROOT, "tests", "golden", "gb_count_kat.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
