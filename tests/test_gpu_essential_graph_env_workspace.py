"""orbm_essential_graph_env's bytes and host waits do not depend on what its pooled workspace held before ("What a call may
assume about its workspace"): the lease site both entries of orbm_essential_graph.hip share, on the envelope path, under the fills of
tests/workspace_cases.py.  What the envelope path adds is written before it is read: every entry of every live tile with a row below
n by k_eg_assemble_env each trial, the running dots by the panel that starts them, x and the ok word by the solve.  No tolerance:
the comparator is the same call in the same process."""
import pytest

import essential_graph_env_scenes as scenes
import workspace_cases as W
from orb_slam2_e_amd import essential_graph as EG

pytestmark = pytest.mark.gpu
KEYS = ("poses", "points", "estimates", "chi2", "trial_log")
NAME = "mid75_free"
_BASE = {}


def run():
    r = EG.optimize_env(scenes.scene(NAME), scenes.ITER1[NAME], want_stats=True)
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
