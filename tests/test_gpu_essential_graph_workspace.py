"""orbm_essential_graph's bytes and host waits do not depend on what its pooled workspace held before ("What a call may
assume about its workspace"): the call's lease site (orbm_essential_graph.hip/orbm_essential_graph) under the fills of
tests/workspace_cases.py, as tests/test_gpu_ba_workspace.py holds orbm_ba.hip's.  The call writes every array before it reads it --
vScw, estimates, measurements and stored errors in k_eg_init, an edge's 161 contributions in k_eg_linearize, the diagonal blocks and b
in k_eg_gather, the whole lower triangle of S in k_eg_assemble, x and the ok word in the solve, every partial in the pass that sums
it.  No tolerance: the comparator is the same call in the same process."""
import pytest

import essential_graph_scenes as scenes
import workspace_cases as W
from orb_slam2_e_amd import essential_graph as EG

pytestmark = pytest.mark.gpu
KEYS = ("poses", "points", "estimates", "chi2", "trial_log")
NAME = "tree40_free"
_BASE = {}


def run():
    r = EG.optimize(scenes.scene(NAME), scenes.ITER1[NAME], want_stats=True)
    return [r[k].tobytes() for k in KEYS] + [repr((r["iterations"], r["trials"], r["results"]))], r["waits"]


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
        assert a == b, f"{NAME} after the fill {fill[0]}: output {k} differs from the baseline"
    assert waits == ref_waits
