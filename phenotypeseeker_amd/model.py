"""The estimator boundary: picklable stand-ins for what the reference stores in
its .pkl -- a fitted GridSearchCV over LogisticRegression(penalty='l1', solver='liblinear') or
Lasso (modeling.py:994-1014, :1075-1085, :1208-1216, :975-979) -- exposing the attributes the
reference reads: predict / predict_proba / score, cv_results_['mean_test_score' |
'std_test_score' | 'params'], best_params_, best_estimator_.coef_ (modeling.py:1226-1247,
:1427-1436; prediction.py:126-129,:168-172).  All fits of a grid search (grid x folds + the
refit) are solved on the GPU in one psk_logreg_l1_fit / psk_lasso_fit launch
(L1LogisticRegression(solver='saga'), the free intercept: psk_logreg_l1_free_fit).  `--penalty L2`
(modeling.py:1001-1002, :1015-1019) maps to RidgeRegression / L2LogisticRegression over
psk_ridge_fit / psk_logreg_l2_fit in the same way, `-bc SVM` (modeling.py:1025-1029) to SVC over
psk_svc_fit, whose folds are scored from the decision values the engine returns, and `-bc DT` (modeling.py:1032-1033) to
DecisionTree over psk_tree_fit under a two-key grid, scored from the leaves the engine returns for every sample, and `-bc RF`
(modeling.py:1030-1031) to RandomForest over psk_forest_fit under RandomizedSearch: scikit-learn's forest and sampler for a
given seed, the host drawing what NumPy's RandomState draws.  `-bc NB` (modeling.py:1034-1035) maps to BernoulliNB over psk_nb_fit /
psk_nb_jll, fitted directly: the reference has no search for it (and cannot complete the branch at all, model_nb.py).  `-bc XGBC`
and `-reg XGBR` map to GradientBoosting over psk_gb_fit / psk_gb_decision, fitted directly too: scikit-learn's gradient boosting,
not XGBoost (the reference names both and has no model for either, model_gb.py).

The classes live in model_linear, model_svc, model_trees, model_nb, model_gb and model_search (the searches, the estimator protocol they ask for
and the export to scikit-learn objects); this module is their one public address.
"""
from .model_gb import GradientBoosting  # noqa: F401
from .model_linear import ElasticNetRegression, L1LogisticRegression, L2LogisticRegression, LassoRegression, RidgeRegression  # noqa: F401
from .model_nb import BernoulliNB  # noqa: F401
from .model_search import GridSearch, RandomizedSearch  # noqa: F401
from .model_svc import SVC, platt_predict_proba, platt_sigmoid_train  # noqa: F401
from .model_trees import RAND_R_MAX, DecisionTree, ForestDraws, ForestTree, RandomForest, Tree  # noqa: F401
