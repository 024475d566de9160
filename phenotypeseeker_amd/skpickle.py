"""Model files as the reference writes them -- joblib-loadable pickles of scikit-learn objects (modeling.py:975-988;
loaded by a plain joblib.load, prediction.py:124-129) -- written WITHOUT importing scikit-learn.

Importing scikit-learn costs 0.3-0.5 s, as much as all the GPU work of a 256-genome `modeling` run.  What a fitted
GridSearchCV / LogisticRegression / Lasso / Ridge / ElasticNet pickles as is its class (module + name) and its attribute
dictionary; the dictionaries of default-constructed estimators are recorded per scikit-learn version in
sklearn_shells.json (tools/make_sklearn_shells.py), the fitted attributes come from this package's own solver.  The
writer emits the pickle opcodes for "object of class <module>.<name> with this state" directly (GLOBAL / NEWOBJ /
BUILD, protocol 2; GLOBAL / argument tuple / REDUCE / state / BUILD for an object that pickles by __reduce__, as the
tree_ of a DecisionTreeClassifier does) and lets the standard pickler serialise the leaves (numbers, strings, numpy
arrays).  When the installed scikit-learn has no template the caller falls back to GridSearch.to_sklearn(), which
imports it.
"""
import json
import math
import os
import pickle


class Shell:
    """Stands for an instance of module.name whose __dict__ will be `state`."""

    def __init__(self, module, name, state):
        self.module, self.name, self.state = module, name, state


class Reduced:
    """Stands for the object that module.name(*args) builds and __setstate__(state) completes: what __reduce__ of an
    extension type returns (sklearn.tree._tree.Tree: args (n_features, n_classes[], n_outputs))."""

    def __init__(self, module, name, args, state):
        self.module, self.name, self.args, self.state = module, name, tuple(args), state


_templates = None


def installed_sklearn_version():
    try:
        from importlib import metadata
        return metadata.version("scikit-learn")
    except Exception:
        return None


def template(cls_name):
    """(module, name, default state) of `cls_name` for the installed scikit-learn, or None."""
    global _templates
    if _templates is None:
        with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "sklearn_shells.json")) as f:
            _templates = json.load(f)
    t = _templates.get(installed_sklearn_version() or "", {}).get(cls_name)
    if t is None:
        return None
    state = {k: (math.nan if v == "nan" else v) for k, v in t["state"].items()}
    return t["module"], t["name"], state


def make(cls_name, **attrs):
    t = template(cls_name)
    if t is None:
        return None
    module, name, state = t
    state.update(attrs)
    return Shell(module, name, state)


def _emit(obj, out):
    if isinstance(obj, Shell):
        out.append(b"c" + obj.module.encode() + b"\n" + obj.name.encode() + b"\n")   # GLOBAL
        out.append(b")\x81")                                                          # EMPTY_TUPLE, NEWOBJ
        _emit(obj.state, out)
        out.append(b"b")                                                              # BUILD
    elif isinstance(obj, Reduced):
        out.append(b"c" + obj.module.encode() + b"\n" + obj.name.encode() + b"\n")   # GLOBAL
        _emit(obj.args, out)                                                          # (a tuple of leaves)
        out.append(b"R")                                                              # REDUCE
        _emit(obj.state, out)
        out.append(b"b")                                                              # BUILD
    elif isinstance(obj, dict) and _has_shell(obj):
        out.append(b"}(")                                                             # EMPTY_DICT, MARK
        for k, v in obj.items():
            _emit(k, out)
            _emit(v, out)
        out.append(b"u")                                                              # SETITEMS
    elif isinstance(obj, list) and _has_shell(obj):
        out.append(b"](")                                                             # EMPTY_LIST, MARK
        for v in obj:
            _emit(v, out)
        out.append(b"e")                                                              # APPENDS
    else:
        # a leaf: the standard pickler's stream without its PROTO header and STOP; its memo indices start from 0 again,
        # which is harmless -- every GET of a fragment refers to a PUT of the same fragment, executed just before
        frag = pickle.dumps(obj, protocol=2)
        assert frag[:2] == b"\x80\x02" and frag[-1:] == b"."
        out.append(frag[2:-1])


def _has_shell(obj):
    if isinstance(obj, (Shell, Reduced)):
        return True
    if isinstance(obj, dict):
        return any(_has_shell(v) for v in obj.values())
    if isinstance(obj, list):
        return any(_has_shell(v) for v in obj)
    return False


def dumps(obj):
    out = [b"\x80\x02"]
    _emit(obj, out)
    out.append(b".")
    return b"".join(out)


# ---- reading a model file for `prediction` without importing scikit-learn ----------------------------------------
class _Stub:
    """Stands in for any scikit-learn class while a model file is unpickled: keeps the attribute dictionary."""

    def __init__(self, *args, **kwargs):
        pass

    def __setstate__(self, state):
        if isinstance(state, dict):
            self.__dict__.update(state)
        elif isinstance(state, tuple) and len(state) == 2:       # (dict, slots)
            for part in state:
                if isinstance(part, dict):
                    self.__dict__.update(part)


class _StubUnpickler(pickle.Unpickler):
    _made = {}

    def find_class(self, module, name):
        if module.split(".")[0] == "joblib":
            # a joblib-wrapped file carries raw array bytes inline behind a NumpyArrayWrapper: read as pickle opcodes they
            # are garbage -- stop here, the caller takes joblib.load
            raise pickle.UnpicklingError("joblib-wrapped arrays: not a plain pickle")
        if module.split(".")[0] == "sklearn":
            key = (module, name)
            if key not in self._made:
                self._made[key] = type(name, (_Stub,), {"__module__": module})
            return self._made[key]
        return super().find_class(module, name)


class LinearModel:
    """What `prediction` needs of a fitted (GridSearchCV of a) linear estimator: predict / predict_proba with the
    expressions scikit-learn evaluates (linear_model/_base.py: X @ coef_.T + intercept_; classes_[scores > 0];
    expit(scores) for the liblinear / one-vs-rest probability of a binary problem)."""

    def __init__(self, coef, intercept, classes):
        import numpy as np
        self.coef_, self.intercept_ = np.asarray(coef, dtype=np.float64), np.asarray(intercept, dtype=np.float64)
        self.classes_ = None if classes is None else np.asarray(classes)

    def _scores(self, X):
        import numpy as np
        X = np.asarray(X, dtype=np.float64)
        if self.classes_ is None:
            return X @ self.coef_.T + self.intercept_ if self.coef_.ndim == 2 else X @ self.coef_ + self.intercept_
        s = X @ self.coef_.T + self.intercept_
        return s.ravel() if s.ndim == 2 and s.shape[1] == 1 else s

    def predict(self, X):
        import numpy as np
        s = self._scores(X)
        if self.classes_ is None:
            return s
        return self.classes_[(s > 0).astype(np.int64)]

    def predict_proba(self, X):
        import numpy as np
        s = self._scores(X)
        # scipy.special.expit, without the overflow warning of exp(-s) at strongly negative scores
        e = np.exp(-np.abs(s))
        p = np.where(s >= 0, 1.0 / (1.0 + e), e / (1.0 + e))
        return np.vstack([1.0 - p, p]).T


def _svc_from_state(est):
    """model.SVC from the attribute dictionary of a fitted two-class dense sklearn.svm.SVC with a linear or rbf kernel and a
    Platt pair: the same decision values, libsvm's vote on a zero and its probability iteration, not the logistic.  None
    for anything else (more classes, sparse fits, other kernels, probability=False, class weights)."""
    import numpy as np
    from .model import SVC
    d = est.__dict__
    classes = d.get("classes_")
    if (classes is None or list(classes) != [0, 1] or d.get("_sparse") or d.get("kernel") not in ("linear", "rbf")
            or len(d.get("_probA", ())) != 1 or len(d.get("_probB", ())) != 1 or d.get("class_weight") is not None):
        return None
    m = SVC(C=d["C"], kernel=d["kernel"], gamma=d["gamma"], tol=d["tol"], max_iter=d["max_iter"], probability=True)
    m.support_ = np.asarray(d["support_"])
    m.support_vectors_ = np.asarray(d["support_vectors_"], dtype=np.float64)
    m.n_support_ = np.asarray(d["_n_support"])
    m.dual_coef_, m.intercept_ = np.asarray(d["dual_coef_"], dtype=np.float64), np.asarray(d["intercept_"], dtype=np.float64)
    m._gamma = float(d["_gamma"])
    m.probA_, m.probB_ = np.asarray(d["_probA"], dtype=np.float64), np.asarray(d["_probB"], dtype=np.float64)
    m.n_features_in_ = int(m.support_vectors_.shape[1])
    return m


def _tree_from_state(est):
    """model.DecisionTree from the attribute dictionary of a fitted two-class, single-output
    sklearn.tree.DecisionTreeClassifier whose tree_ came through the stub (Tree.__getstate__: max_depth, node_count, nodes,
    values): predict / predict_proba walk the node arrays in NumPy.  None for anything else."""
    import numpy as np
    from .model import DecisionTree, Tree
    d = est.__dict__
    classes, tree = d.get("classes_"), d.get("tree_")
    if (classes is None or getattr(classes, "ndim", 0) != 1 or list(classes) != [0, 1] or d.get("n_outputs_") != 1 or tree is None
            or not {"nodes", "values", "max_depth"} <= set(getattr(tree, "__dict__", {}))):
        return None
    values = np.asarray(tree.values)
    if values.ndim != 3 or values.shape[1:] != (1, 2) or np.any(tree.nodes["missing_go_to_left"]):
        return None
    m = DecisionTree(criterion=d.get("criterion", "gini"), max_depth=d.get("max_depth"))
    m.tree_ = Tree._from_sklearn_state(int(d["n_features_in_"]), tree.__dict__)
    m.n_features_in_ = int(d["n_features_in_"])
    return m


def _forest_from_state(est):
    """model.RandomForest from the attribute dictionary of a fitted two-class, single-output
    sklearn.ensemble.RandomForestClassifier whose estimators_ came through the stub: every tree as _tree_from_state reads
    it.  None for anything else."""
    from .model import RandomForest
    d = est.__dict__
    classes, trees = d.get("classes_"), d.get("estimators_")
    if classes is None or getattr(classes, "ndim", 0) != 1 or list(classes) != [0, 1] or d.get("n_outputs_") != 1 or not trees:
        return None
    models = [_tree_from_state(t) for t in trees]
    if any(m is None for m in models):
        return None
    m = RandomForest(n_estimators=d.get("n_estimators", len(models)), criterion=d.get("criterion", "gini"), max_depth=d.get("max_depth"),
                     min_samples_split=d.get("min_samples_split", 2), min_samples_leaf=d.get("min_samples_leaf", 1),
                     max_features=d.get("max_features", "sqrt"), bootstrap=d.get("bootstrap", True), random_state=d.get("random_state"))
    m.estimators_ = models
    m.n_features_in_ = int(d["n_features_in_"])
    return m


def _nb_from_state(est):
    """model.BernoulliNB from the attribute dictionary of a fitted two-class sklearn.naive_bayes.BernoulliNB with the default
    parameters: its counts, and the two log attributes as the file holds them.  None for anything else."""
    import numpy as np
    from .model import BernoulliNB
    d = est.__dict__
    classes, flp, clp = d.get("classes_"), d.get("feature_log_prob_"), d.get("class_log_prior_")
    if classes is None or getattr(classes, "ndim", 0) != 1 or list(classes) != [0, 1] or flp is None or clp is None:
        return None
    try:
        m = BernoulliNB(**{k: d[k] for k in BernoulliNB._DEFAULTS})
    except (KeyError, ValueError):      # other parameters than the defaults: scikit-learn itself
        return None
    m.feature_count_ = np.asarray(d["feature_count_"], dtype=np.float64)
    m.class_count_ = np.asarray(d["class_count_"], dtype=np.float64)
    m.feature_log_prob_, m.class_log_prior_ = np.asarray(flp, dtype=np.float64), np.asarray(clp, dtype=np.float64)
    if m.feature_log_prob_.shape != (2, int(d["n_features_in_"])) or m.class_log_prior_.shape != (2,):
        return None
    m.n_features_in_ = int(d["n_features_in_"])
    return m


def load_linear_package(path):
    """The model package of `path` ({'model', 'kmers', 'pca', 'pred_scale'}) with 'model' as a LinearModel -- for files
    that are plain pickles of a (grid search over a) binary linear classifier or a linear regressor, which is what
    `modeling` writes; a two-class SVC with a Platt pair comes back as model.SVC (_svc_from_state), a two-class decision tree
    as model.DecisionTree (_tree_from_state), a two-class random forest as model.RandomForest (_forest_from_state), a two-class
    BernoulliNB() as model.BernoulliNB (_nb_from_state).  A package with 'pca' true (`modeling --pca`) keeps its 'PCs_to_keep' and
    comes back with 'scaler' and 'pca_model' as model_pca.StandardScaler and model_pca.PCA (model_pca.from_state).  None for
    anything else (joblib-wrapped arrays, multi-class models, other estimators, a scaler or PCA with other than the default
    parameters): the caller then takes joblib.load and scikit-learn itself."""
    try:
        with open(path, "rb") as f:
            pkg = _StubUnpickler(f).load()
        if not isinstance(pkg, dict) or "model" not in pkg:
            return None
        if pkg.get("pca"):
            from . import model_pca
            if not {"scaler", "pca_model", "PCs_to_keep"} <= set(pkg):
                return None
            pair = model_pca.from_state(pkg["scaler"], pkg["pca_model"])
            if pair is None:
                return None
            pkg = dict(pkg, scaler=pair[0], pca_model=pair[1])
        m = pkg["model"]
        est = getattr(m, "best_estimator_", m)
        kind = type(est).__name__
        coef, icpt = getattr(est, "coef_", None), getattr(est, "intercept_", None)
        if kind == "DecisionTreeClassifier":
            model = _tree_from_state(est)
            if model is None:
                return None
            return dict(pkg, model=model)
        if kind == "RandomForestClassifier":
            model = _forest_from_state(est)
            if model is None:
                return None
            return dict(pkg, model=model)
        if kind == "BernoulliNB":
            model = _nb_from_state(est)
            if model is None:
                return None
            return dict(pkg, model=model)
        if kind != "SVC" and (coef is None or icpt is None):   # (an SVC keeps its support vectors, coef_ is derived)
            return None
        if kind in ("LogisticRegression",):
            classes = getattr(est, "classes_", None)
            if classes is None or len(classes) != 2 or getattr(coef, "shape", (0,))[0] != 1:
                return None
            # a binary model saved with multi_class='multinomial' has softmax([-d, d]) = expit(2 d) probabilities in
            # scikit-learn, not expit(d): leave it to joblib.load + scikit-learn
            if getattr(est, "multi_class", "auto") not in ("auto", "ovr", "deprecated", "warn"):
                return None
            model = LinearModel(coef, icpt, classes)
        elif kind in ("Lasso", "Ridge", "ElasticNet"):
            model = LinearModel(coef, icpt, None)
        elif kind == "SVC":
            model = _svc_from_state(est)
            if model is None:
                return None
        else:
            return None
        out = dict(pkg)
        out["model"] = model
        return out
    except Exception:   # noqa: BLE001 -- any surprise: the ordinary loader decides
        return None
