"""The dry-built launch plans are the ones tests/golden/plan_fingerprint.json pins (tests/tools/plan_fingerprint.py, no GPU): config 2's
fused train step and inference plan, the F = 40 train step, the autograd front end, a SyncBN train step with the exchange forced at
world 1, the segments of a gated inference plan (EDM, entropy and top-probability gates, the latter two also with ADDK_FUSE_GATE=0),
a validation plan with its scoring heads and with the stand-alone fallback of 7 classes, an exit-profile plan, the label-map plans
(Segmenter at the final exit with a table and at exit 0, the EDM-gated and the entropy / top-probability gated plans with
output='labels', the latter also with ADDK_FUSE_GATE=0), each with and without level batching.
Every command of every list is compared: order, stream, waits, events, regions and each argument byte, with addresses replaced by
(allocation, offset); also the plan's size and its buffers.  A refactor of the planner leaves all of it as it is; a change that is
meant to alter a plan re-records the fixture with the tool and says so."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests', 'tools'))
import plan_fingerprint as FP     # noqa: E402


def test_dry_built_plans_equal_the_recorded_fingerprints():
    with open(FP.OUT) as f:
        want = json.load(f)
    assert len(want) == len(FP.PLANS) * len(FP.ENVS)
    diff = FP.differences(FP.fingerprints(), want)
    assert not diff, '\n'.join(diff)
