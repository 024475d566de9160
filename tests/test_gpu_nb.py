"""GPU tests of the naive-Bayes path (-m gpu): psk_nb_fit, psk_nb_jll, model.BernoulliNB on the device and `-bc NB` end to end.
Yardsticks: scikit-learn's recorded fits (tests/golden/nb_kat.npz, tools/gen_nb_golden.py) and the NumPy restatement
(tests/nb_restated.py).  Counts and the log attributes are ==.  The joint log-likelihood is == the restatement, which adds in
the order include/psk.h states, and within the derived bound of scikit-learn, which adds the same terms in another order
(nb_restated.py: tol_ic = 2 (p + 2) 2^-53 (sum_j x_ij |delta_cj| + |class_log_prior_c| + |neg_sum_c|))."""
import os

import numpy as np
import pytest

import nb_restated as R

pytestmark = pytest.mark.gpu

EINVAL, ERANGE = -1, -4


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
def restated(fx):
    """Per design and case the restatement's (fc, cc, jll) and the bound, from the fixture's own log attributes; once."""
    out = []
    for D, cases in zip(fx.designs, fx.cases):
        Xb = D["X"] != 0
        out.append([dict(zip(("fc", "cc"), R.counts(Xb, D["y"], c["train"])), jll=R.jll_in_order(Xb, c["flp"], c["clp"]),
                         tol=R.jll_tolerance(Xb, c["flp"], c["clp"])) for c in cases])
    return out


def terms(cases):
    """(delta[m][2][p], class_log_prior[m][2], neg_sum[m][2]) of the recorded models."""
    pairs = [R.jll_terms(c["flp"]) for c in cases]
    return np.stack([d for d, _ in pairs]), np.stack([c["clp"] for c in cases]), np.stack([s for _, s in pairs])


def test_counts_of_all_fits_in_one_launch(ctx, fx, restated):
    """Per design ONE psk_nb_fit call carries the all-sample fit and every fold-masked fit."""
    for d, (D, cases) in enumerate(zip(fx.designs, fx.cases)):
        fc, cc = ctx.nb_fit(D["X"], D["y"], D["fold"], [c["held"] for c in cases])
        assert fc.shape == (4, 2, D["p"]) and cc.shape == (4, 2) and fc.dtype == np.int32 and cc.dtype == np.int32
        for k, (c, r) in enumerate(zip(cases, restated[d])):
            assert np.array_equal(fc[k], r["fc"]) and np.array_equal(cc[k], r["cc"]), (d, k)
            assert np.array_equal(fc[k], c["fc"]) and np.array_equal(cc[k], c["cc"]), (d, k)
            flp, clp = R.log_attributes(fc[k], cc[k])
            assert np.array_equal(flp, c["flp"]) and np.array_equal(clp, c["clp"]), (d, k)
        # the order of the fits is the caller's, and a fit alone gives the same counts
        fc1, cc1 = ctx.nb_fit(D["X"], D["y"], D["fold"], [2])
        assert np.array_equal(fc1[0], fc[3]) and np.array_equal(cc1[0], cc[3]), d


def test_jll_of_several_models_in_one_call(ctx, fx, restated):
    from phenotypeseeker_amd import model as M
    worst = 0.0
    for d, (D, cases) in enumerate(zip(fx.designs, fx.cases)):
        delta, prior, neg = terms(cases)
        jll = ctx.nb_jll(D["X"], delta, prior, neg)
        assert jll.shape == (4, D["n"], 2)
        for k, (c, r) in enumerate(zip(cases, restated[d])):
            assert np.array_equal(jll[k], r["jll"]), (d, k)                       # the stated order, bit for bit
            m = M.BernoulliNB()._set_counts(c["fc"], c["cc"])
            assert np.array_equal(jll[k], m._joint_log_likelihood(D["X"])), (d, k)     # the estimator's host path
            assert np.array_equal(jll[k], m._joint_log_likelihood(D["X"], ctx)), (d, k)
            err = np.abs(jll[k] - c["jll"])
            worst = max(worst, float((err / r["tol"]).max()))
            print("design %d case %d: max |jll - sklearn| / bound = %.4f" % (d, k, float((err / r["tol"]).max())))
            assert np.all(err <= r["tol"]), (d, k, float((err / r["tol"]).max()))      # scikit-learn, another order
            band = r["tol"].sum(axis=1)
            assert np.all(np.abs(m.predict_proba(D["X"], ctx) - c["proba"]) <= band[:, None]), (d, k)
            clear = np.abs(c["jll"][:, 0] - c["jll"][:, 1]) > band
            assert np.mean(~clear) <= 0.01 and np.array_equal(m.predict(D["X"], ctx)[clear], c["pred"][clear]), (d, k)
        # one model per call, and rows that share their word with other samples (or with none): identical bits
        one = ctx.nb_jll(D["X"], delta[2], prior[2], neg[2])
        assert one.shape == (D["n"], 2) and np.array_equal(one, jll[2]), d
        lo, hi = min(3, D["n"] - 1), min(D["n"], 70)
        assert np.array_equal(ctx.nb_jll(D["X"][lo:hi], delta[:2], prior[:2], neg[:2]), jll[:2, lo:hi]), d
        assert np.array_equal(ctx.nb_jll(D["X"][-1:], delta[1], prior[1], neg[1]), jll[1, -1:]), d
    print("psk_nb_jll against scikit-learn: worst share of the bound %.4f" % worst)


def test_the_design_past_4096_samples_passes(ctx, fx, restated):
    D, cases = fx.designs[5], fx.cases[5]
    assert (D["n"], D["p"]) == (4100, 5)
    from phenotypeseeker_amd import model as M
    m = M.BernoulliNB().fit(D["X"], D["y"], ctx)
    assert np.array_equal(m.feature_count_, cases[0]["fc"]) and np.array_equal(m.class_count_, cases[0]["cc"])
    assert np.array_equal(m.feature_log_prob_, cases[0]["flp"]) and np.array_equal(m.class_log_prior_, cases[0]["clp"])
    assert np.array_equal(m._joint_log_likelihood(D["X"], ctx), restated[5][0]["jll"])
    assert np.array_equal(m.predict(D["X"], ctx), m.predict(D["X"])) and m.score(D["X"], D["y"], ctx) == m.score(D["X"], D["y"])


def test_refusals_leave_the_context_usable(ctx, fx):
    from phenotypeseeker_amd._lib import PskError
    D, c = fx.designs[2], fx.cases[2][0]
    delta, neg = R.jll_terms(c["flp"])
    good_fit = lambda: ctx.nb_fit(D["X"], D["y"], D["fold"], [-1, 1])
    good_jll = lambda: ctx.nb_jll(D["X"], delta, c["clp"], neg)
    want_fc, want_jll = good_fit()[0], good_jll()
    X2 = D["X"].copy()
    X2[64, 66] = 2.0                                            # a count is not a presence bit
    with pytest.raises(PskError) as e:
        ctx.nb_fit(X2, D["y"], D["fold"], [-1])
    assert e.value.code == EINVAL and "psk_nb_fit" in str(e.value)
    assert np.array_equal(good_fit()[0], want_fc)
    with pytest.raises(PskError) as e:
        ctx.nb_jll(X2, delta, c["clp"], neg)
    assert e.value.code == EINVAL and "psk_nb_jll" in str(e.value)
    assert np.array_equal(good_jll(), want_jll)
    one_class_fold = np.where(D["y"] == 1, 0, 1).astype(np.int32)      # holding fold 0 out leaves class 0 alone
    with pytest.raises(PskError) as e:
        ctx.nb_fit(D["X"], D["y"], one_class_fold, [-1, 0])
    assert e.value.code == EINVAL and "one class" in str(e.value)
    assert np.array_equal(good_fit()[0], want_fc)
    with pytest.raises(PskError) as e:
        ctx.nb_fit(D["X"], np.zeros(D["n"], dtype=np.int32), D["fold"], [-1])
    assert e.value.code == EINVAL
    # past the stated limits: samples (a word of 64 per grid row, 65535 rows) and models per call
    big = 65535 * 64 + 1
    with pytest.raises(PskError) as e:
        ctx.nb_fit(np.zeros((big, 1), dtype=np.float32), np.arange(big) % 2, np.zeros(big, dtype=np.int32), [-1])
    assert e.value.code == ERANGE
    with pytest.raises(PskError) as e:
        ctx.nb_jll(np.zeros((big, 1), dtype=np.float32), np.zeros((2, 1)), np.zeros(2), np.zeros(2))
    assert e.value.code == ERANGE
    with pytest.raises(PskError) as e:
        ctx.nb_jll(np.zeros((1, 1), dtype=np.float32), np.zeros((65536, 2, 1)), np.zeros((65536, 2)), np.zeros((65536, 2)))
    assert e.value.code == ERANGE
    assert np.array_equal(good_jll(), want_jll) and np.array_equal(good_fit()[0], want_fc)


def _run(tmp, argv):
    from phenotypeseeker_amd.cli import build_parser
    os.chdir(tmp)
    args = build_parser().parse_args(argv)
    args.func(args)


def test_cli_end_to_end(tmp_path, monkeypatch):
    """PSK_NB=1 phenotypeseeker modeling -bc NB writes the three NB files; the .pkl goes through `phenotypeseeker prediction` on
    the same samples, by the stub reader (psk_nb_jll through the open context) and by joblib (scikit-learn itself), and
    reproduces the summary's training predictions with identical output files."""
    from helpers import load_dataset
    from test_host_modeling import _write_dataset
    monkeypatch.setenv("PSK_NB", "1")
    ds = load_dataset("ds_omitB")
    names = ["summary_of_NB_analysis_Pheno.txt", "k-mers_and_coefficients_in_NB_model_Pheno.txt", "NB_model_Pheno.pkl"]
    wd = tmp_path / "run"
    wd.mkdir()
    _write_dataset(ds, str(wd))
    _run(wd, ["modeling", "data.pheno", "-bc", "NB", "--omit_B_correction", "--n_kmers", "100"])
    for nm in names:
        assert (wd / nm).exists(), nm
    assert not (wd / "log_reg_model_Pheno.pkl").exists()
    summary = (wd / names[0]).read_text()
    assert "Parameters:" not in summary and "Grid scores" not in summary and "Best parameters" not in summary
    block = summary.split("Sample_ID Acutal_phenotype Predicted_phenotype\n")[1].split("\n\n")[0]
    trained = {ln.split()[0]: ln.split()[2] for ln in block.splitlines()}
    assert len(trained) == sum(1 for v in ds["pheno"] if v != "NA")
    coef_lines = (wd / names[1]).read_text().splitlines()
    assert coef_lines[0] == "K-mer\tcoef._in_NB_model\tNo._of_samples_with_k-mer\tSamples_with_k-mer" and len(coef_lines) > 1
    assert all(ln.split("\t")[1] == "NA" for ln in coef_lines[1:])
    os.chdir(wd)
    with open("samples.txt", "w") as f:
        for line in open("data.pheno").read().splitlines()[1:]:
            if line.strip():
                f.write("\t".join(line.split()[:2]) + "\n")
    with open("phenos.txt", "w") as f:
        f.write("Pheno\t%s\n" % names[2])
    outs = []
    for flag in ("0", "1"):
        monkeypatch.setenv("PSK_JOBLIB_LOAD", flag)
        _run(wd, ["prediction", "samples.txt", "phenos.txt"])
        out = open("predictions_Pheno.txt").read().splitlines()
        assert out[0] == "Sample_ID\tpredicted_phenotype\tprobability_for_predicted_class"
        pred = {ln.split("\t")[0]: ln.split("\t")[1] for ln in out[1:]}
        assert {k: pred[k] for k in trained} == trained
        for ln in out[1:]:
            assert 0.0 <= float(ln.split("\t")[2]) <= 1.0
        outs.append(out)
    assert outs[0] == outs[1]
