"""orbm_refine_sim3_candidates' bytes and host waits do not depend on what its pooled workspace held before ("What a call
may assume about its workspace"): the call's lease site (orbm_refine_sim3.hip/orbm_refine_sim3_candidates) under the fills of
tests/workspace_cases.py, as tests/test_gpu_essential_graph_workspace.py holds orbm_essential_graph.hip's.  The call writes every
array before it reads it -- every query in k_project_pair_jobs, best and idx of every query in k_win_best_jobs, found12 of every
keypoint, the first n entries of the pair arrays and of the list, n itself and the two counts in k_refine_gather, the first n kept
bytes and the result in k_sim3_optimize -- and the host reads n entries, not n1.  The batch is the ragged one: three attempts with
different n2, one of them with fewer than ten pairs left.  No tolerance: the comparator is the same call in the same process."""
import pytest

import refine_sim3_scenes as scenes
import workspace_cases as W
from test_gpu_refine_sim3 import as_bytes, call

pytestmark = pytest.mark.gpu
NAME = "ragged3"
_BASE = {}


def run():
    fixed, atts = scenes.batches()[NAME]
    out, waits = call(atts, fixed)                  # orb_slam2_e_amd.sim3.refine_sim3_candidates
    return [as_bytes(r) for r in out], waits


def baseline():
    if NAME not in _BASE:
        _BASE[NAME] = run()
    return _BASE[NAME]


@pytest.mark.parametrize("fill", W.FILLS, ids=[f[0] for f in W.FILLS])
def test_stale_arena_contents_change_nothing(fill):
    ref, ref_waits = baseline()
    _, word, as_next = fill
    nw, _ = W.fill_workspaces(word, as_next)
    assert nw >= 1
    out, waits = run()
    for k, (a, b) in enumerate(zip(out, ref)):
        assert a == b, f"{NAME} after the fill {fill[0]}: attempt {k} differs from the baseline"
    assert waits == ref_waits == 1
