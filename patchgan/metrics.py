from patchgan_amd.metrics import *  # noqa: F401,F403
from patchgan_amd.metrics import SegCounts, scores, report, jsonable, BestTracker  # noqa: F401
