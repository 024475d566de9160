"""GPU tests of the C-SVC path (-m gpu): psk_svc_fit, model.SVC behind GridSearch and `-bc SVM` end to end, against
scikit-learn's own fits recorded in tests/golden/svm_kat.npz (tools/gen_svm_golden.py).  Three tiers:
  exact path    the solver restates libsvm's Solver::Solve without shrinking step for step, so iteration counts are EQUAL
                and values agree to 1e-6 relative (the project's coefficient tolerance), fits stopped at
                max_iter included;
  certificate   whatever the path, a fit that stopped before max_iter satisfies libsvm's stopping rule, recomputed here
                from the exact kernel matrix, within twice the excess scikit-learn's own solutions show (measured by the
                generator: rounding of G accumulated over up to 1000 updates);
  reference     against SVC(shrinking=True), the reference's actual call, within twice the largest on / off deviation the
                generator found among converged fits.  Fits the reference stopped at max_iter on and whose two records
                differ are the documented departure (libsvm's shrinking heuristic permutes the index
                order and is not restated); they are listed, not compared."""
import os

import numpy as np
import pytest

import svm_restated as R

pytestmark = pytest.mark.gpu

PATH_RTOL = 1e-6


@pytest.fixture(scope="module")
def ctx():
    from phenotypeseeker_amd.engine import PskContext
    c = PskContext(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def fx():
    return R.Fixture()


@pytest.fixture(scope="module")
def gpu_fits(ctx, fx):
    """Every fit of the fixture through psk_svc_fit, one launch per (design, kernel): [(dual, rho, dec, iters)] by fit."""
    out = [None] * len(fx.fits)
    groups = {}
    for j, f in enumerate(fx.fits):
        groups.setdefault((f["design"], f["kernel"]), []).append(j)
    for (d, kern), js in groups.items():
        D = fx.designs[d]
        dual, rho, dec, iters = ctx.svc_fit(D["X"], D["y"], D["folds"], [fx.fits[j]["C"] for j in js],
                                            [fx.fits[j]["fold"] for j in js], kernel=kern,
                                            fit_gamma=[fx.fits[j]["gamma"] for j in js], tol=fx.tol, max_iter=fx.max_iter)
        for k, j in enumerate(js):
            out[j] = (dual[k], float(rho[k]), dec[k], int(iters[k]))
    print("psk_svc_fit: %d fits in %d launches" % (len(out), len(groups)))
    return out


def _close(got, want):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max()) <= PATH_RTOL * max(1.0, float(np.abs(want).max()))


def test_exact_path_tier(fx, gpu_fits):
    """iters_out equals n_iter_ of SVC(shrinking=False) on every admissible linear fit; duals, rho and the decision values
    of all n samples within 1e-6 relative on both kernels.  The rbf kernel's iteration agreement is counted and printed:
    the device's exp is not glibc's, and a float entry of Q may round the other way."""
    n_lin = n_rbf = rbf_same_iters = capped = 0
    worst = 0.0
    for f, (dual, rho, dec, iters) in zip(fx.fits, gpu_fits):
        if not f["admissible"]:
            continue
        off = f["off"]
        tr = fx.train_mask(f)
        assert np.all(dual[~tr] == 0.0), "duals of samples the fit did not train on must be 0"
        if f["kernel"] == "linear":
            n_lin += 1
            capped += off["iters"] >= fx.max_iter
            assert iters == off["iters"], (f["design"], f["C"], f["fold"], iters, off["iters"])
        else:
            n_rbf += 1
            rbf_same_iters += iters == off["iters"]
        worst = max(worst, float(np.abs(dec - off["dec"]).max()) / max(1.0, float(np.abs(off["dec"]).max())))
        assert _close(dual, off["dual"]) and _close(rho, off["rho"]) and _close(dec, off["dec"]), \
            (f["design"], f["kernel"], f["C"], f["fold"], iters, off["iters"])
    print("exact path: %d linear fits (%d stopped at max_iter) with equal iteration counts; rbf: %d of %d equal; "
          "largest relative deviation of a decision value %.3g" % (n_lin, capped, rbf_same_iters, n_rbf, worst))
    assert n_lin > 100 and capped > 0 and n_rbf > 30
    assert any(f["fold"] >= 0 for f in fx.fits) and any(f["fold"] < 0 for f in fx.fits)


def test_certificate_tier(fx, gpu_fits):
    """Every fit that stopped before max_iter: 0 <= alpha <= C, the sign of a dual is its class's, and |y'a| / C and the
    recomputed Gmax + Gmax2 - tol stay below twice what scikit-learn's own recorded solutions show."""
    gap_slack, eq_slack = 2.0 * float(fx.z["cert_gap_excess"]), 2.0 * float(fx.z["cert_eq_excess"])
    kmats = {}
    checked, worst_gap, worst_eq = 0, -np.inf, 0.0
    for f, (dual, rho, dec, iters) in zip(fx.fits, gpu_fits):
        if iters >= fx.max_iter:
            continue
        D = fx.designs[f["design"]]
        key = (f["design"], f["kernel"])
        if key not in kmats:
            kmats[key] = R.kernel_matrix(D["X"], f["kernel"], f["gamma"])
        tr = fx.train_mask(f)
        y = D["y"]
        assert np.all(np.abs(dual) <= f["C"]), "alpha above C"
        assert np.all(dual[y == 0] >= 0.0) and np.all(dual[y == 1] <= 0.0), "alpha below 0"
        gap, eq = R.optimality(kmats[key][np.ix_(tr, tr)], y[tr], dual[tr], f["C"])
        worst_gap, worst_eq = max(worst_gap, gap - fx.tol), max(worst_eq, eq / f["C"])
        assert gap - fx.tol <= gap_slack, (key, f["C"], f["fold"], gap - fx.tol, gap_slack)
        assert eq / f["C"] <= eq_slack, (key, f["C"], f["fold"], eq / f["C"], eq_slack)
        checked += 1
    print("certificate: %d converged fits; Gmax + Gmax2 - tol at most %.3g (allowed %.3g), |y'a| / C at most %.3g (allowed %.3g)"
          % (checked, worst_gap, gap_slack, worst_eq, eq_slack))
    assert checked > 150


def test_reference_tier(fx, gpu_fits):
    """Against SVC(shrinking=True), what the reference calls: every fit it converged on, and the capped ones whose two
    records are identical."""
    bound = 2.0 * float(fx.z["conv_on_off_dev"])
    compared, departures, worst = 0, [], 0.0
    for f, (dual, rho, dec, iters) in zip(fx.fits, gpu_fits):
        on = f["on"]
        if on["iters"] >= fx.max_iter and not f["same"]:
            departures.append((f["design"], f["kernel"], f["C"], f["fold"]))
            continue
        dev = float(np.abs(dec - on["dec"]).max())
        worst = max(worst, dev)
        assert dev <= bound, (f["design"], f["kernel"], f["C"], f["fold"], dev, bound)
        sure = np.abs(on["dec"]) > bound
        assert np.array_equal((dec <= 0)[sure], (on["dec"] <= 0)[sure])
        compared += 1
    print("reference: %d fits within %.3g of SVC(shrinking=True) (largest deviation %.3g)" % (compared, bound, worst))
    print("skipped, the documented departure (stopped at max_iter with the shrinking heuristic's own index order): %d fits" % len(departures))
    for d in departures:
        print("   design %d %s C=%g fold %d" % d)
    assert compared > 150


def test_refuses_what_it_cannot_hold(ctx):
    """More than 4096 samples: an error code, not another route; a fit whose training samples are of one class too."""
    from phenotypeseeker_amd._lib import PskError
    X = np.zeros((4097, 3), dtype=np.float32)
    y = (np.arange(4097) % 2).astype(np.int32)
    with pytest.raises(PskError) as e:
        ctx.svc_fit(X, y, np.zeros(4097, np.int32), [1.0], [-1])
    assert e.value.code == -4
    with pytest.raises(PskError):
        ctx.svc_fit(np.eye(4, dtype=np.float32), [0, 0, 1, 1], [0, 0, 1, 1], [1.0], [1])


def test_counts_design_takes_the_dense_gram(ctx):
    """A design that is not 0/1 (--real_counts): f64 dot products instead of popcounts, the same solver."""
    rng = np.random.default_rng(5)
    X = rng.integers(0, 4, (60, 25)).astype(np.float64)
    y = (X[:, 0] + X[:, 1] + rng.integers(0, 3, 60) > 4).astype(int)
    folds = np.arange(60) % 3
    Cs, ff = [0.01, 0.1, 1.0, 0.1], [-1, -1, 0, 2]
    for kern, g in (("linear", 0.0), ("rbf", 0.02)):
        dual, rho, dec, iters = ctx.svc_fit(X, y, folds, Cs, ff, kernel=kern, fit_gamma=g, tol=1e-4, max_iter=1000)
        for k in range(len(Cs)):
            rd, rr, rdec, rit = R.fit(X, y, folds != ff[k], Cs[k], kern, g, 1e-4, 1000)
            if kern == "linear":
                assert iters[k] == rit
            assert _close(dual[k], rd) and _close(rho[k], rr) and _close(dec[k], rdec), (kern, k, iters[k], rit)


def test_grid_search_scores_equal_scikit_learn(ctx, fx):
    """GridSearch(SVC) scores the folds from dec_out: split scores, means, ranks and the best C equal the recorded cv_results_ of
    GridSearchCV(SVC(shrinking=False)) -- the same path, so the same predictions -- and those of the reference's own call
    (shrinking=True) on the designs where the generator found the two records equal."""
    from phenotypeseeker_amd import model as M
    n_designs = distinct = with_on = 0
    for d, D in enumerate(fx.designs):
        tag = "gs%d_" % d
        if tag + "mean_off" not in fx.z:
            continue
        splits = fx.z[tag + "splits_off"]
        gs = M.GridSearch(M.SVC(kernel="linear", probability=True, tol=fx.tol, max_iter=float(fx.max_iter)), "C", list(fx.Cs), splits.shape[1])
        gs.fit(D["X"], D["y"], ctx)
        records = [("off", "shrinking=False")] + ([("on", "shrinking=True")] if bool(fx.z[tag + "equal"]) else [])
        for rec, what in records:
            for f in range(splits.shape[1]):
                assert np.array_equal(gs.cv_results_["split%d_test_score" % f], fx.z[tag + "splits_" + rec][:, f]), (d, what, f)
            assert np.array_equal(gs.cv_results_["mean_test_score"], fx.z[tag + "mean_" + rec]), (d, what)
            assert np.array_equal(gs.cv_results_["rank_test_score"], fx.z[tag + "rank_" + rec]), (d, what)
            assert gs.best_params_["C"] == float(fx.z[tag + "best_C_" + rec]), (d, what)
        n_designs += 1
        with_on += len(records) == 2
        distinct = max(distinct, len(set(gs.cv_results_["mean_test_score"].tolist())))
        print("design %d (%d x %d): %d distinct mean scores, best C %g, compared with %s"
              % (d, D["n"], D["p"], len(set(gs.cv_results_["mean_test_score"].tolist())), gs.best_params_["C"],
                 " and ".join(w for _, w in records)))
        # the refit is the all-sample fit of the fixture at the chosen C
        best = [f for f in fx.fits if f["design"] == d and f["fold"] < 0 and f["kernel"] == "linear" and f["C"] == gs.best_params_["C"]][0]
        be = gs.best_estimator_
        assert int(be.n_iter_[0]) == best["off"]["iters"]
        assert _close(-be.decision_function(D["X"]), best["off"]["dec"])
        p = gs.predict_proba(D["X"])
        assert p.shape == (D["n"], 2) and np.allclose(p.sum(axis=1), 1.0) and np.all((p > 0) & (p < 1))
    assert n_designs >= 2 and with_on >= 1 and with_on < n_designs and distinct >= 7


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def test_cli_end_to_end(tmp_path, monkeypatch):
    """PSK_SVM=1 phenotypeseeker modeling -bc SVM writes the three SVM files; the .pkl goes through `phenotypeseeker
    prediction` on the same samples and reproduces the summary's training predictions; a second run writes the same bytes
    (the Platt pair comes from a deterministic split)."""
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    monkeypatch.setenv("PSK_SVM", "1")
    ds = load_dataset("ds_omitB")
    names = ["summary_of_SVM_analysis_Pheno.txt", "k-mers_and_coefficients_in_SVM_model_Pheno.txt", "SVM_model_Pheno.pkl"]
    runs = []
    for rep in range(2):
        wd = tmp_path / ("run%d" % rep)
        wd.mkdir()
        _write_dataset(ds, str(wd))
        _run(wd, ["modeling", "data.pheno", "-bc", "SVM", "--kernel", "linear", "--omit_B_correction", "--n_kmers", "100"])
        for nm in names:
            assert (wd / nm).exists(), nm
        assert not (wd / "log_reg_model_Pheno.pkl").exists()
        runs.append(wd)
    for nm in names:
        assert (runs[0] / nm).read_bytes() == (runs[1] / nm).read_bytes(), "%s differs between two runs" % nm
    wd = runs[0]
    summary = (wd / names[0]).read_text()
    assert "Parameters:\nSVC(kernel='linear', max_iter=1000, probability=True, tol=0.0001)\n" in summary
    assert "Grid scores (mean accuracy) on development set:" in summary
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    assert len(trained) == sum(1 for v in ds["pheno"] if v != "NA")
    coef_lines = (wd / names[1]).read_text().splitlines()
    assert coef_lines[0] == "K-mer\tcoef._in_SVM_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" and len(coef_lines) > 1
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    _run(wd, ["prediction", "samples.txt", "phenos.txt"])
    out = open("predictions_Pheno.txt").read().splitlines()
    assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class"
    pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
    assert {k: pred[k] for k in trained} == trained
    for ln in out[1:]:
        assert 0.0 <= float(ln.split("\t")[2]) <= 1.0
