from patchgan_amd.metrics import *  # noqa: F401,F403
from patchgan_amd.metrics import SegCounts, scores, report, jsonable, BestTracker  # noqa: F401
from patchgan_amd.metrics import SegHist, curve, report_curve, best_threshold, check_bins  # noqa: F401
