"""Reference import path ``utils.eval_utils`` -> lstc_vad_amd.metrics (``eval`` = frame-level ROC-AUC, :139-143; the PR / AP,
thresholded and score-statistic metrics and the per-class table ``eval_each_part``, :12-122 and :145-148, without sklearn).
``cal_f1``, ``eval_classification*`` and the pyplot import stay out."""
from lstc_vad_amd.metrics import eval, roc_auc  # noqa: F401,A004
from lstc_vad_amd.metrics import (cal_accuracy, cal_AP, cal_f_measure, cal_false_alarm, cal_false_neg,  # noqa: F401
                                  cal_geometric_mean, cal_MCC, cal_pAUC, cal_pr_auc, cal_precision, cal_recall, cal_rmse,
                                  cal_score_gap, cal_sensitivity, cal_specific, eval_each_part)

cal_auc = roc_auc
