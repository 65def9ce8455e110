"""orbm_bundle_adjustment's bytes and host waits do not depend on what its pooled workspace held before ("What a call may
assume about its workspace"): the call's lease site (orbm_ba.hip/orbm_bundle_adjustment) under the fills of
tests/workspace_cases.py, as tests/test_gpu_workspace_contents.py holds the other sites.  The call writes every array before it
reads it -- estimates, stored errors and levels in k_ba_init, the vertex sets in k_ba_activate, every block of the system in the
pass that builds it; the reduced matrix is read below its diagonal only, where k_ba_schur has written.  No tolerance: the
comparator is the same call in the same process."""
import numpy as np
import pytest

import ba_scenes
import workspace_cases as W
from orb_slam2_e_amd import bundle

pytestmark = pytest.mark.gpu
KEYS = ("poses", "points", "erase", "not_included", "poses_d", "points_d", "chi2", "level", "trial_log")
_BASE = {}


def run(name):
    _, g, opt = ba_scenes.scenes([name])[0]
    r = bundle.run(g, opt, want_stats=True)
    return [r[k].tobytes() for k in KEYS] + [repr((r["iterations"], r["trials"], r["results"], r["stopped"]))], r["waits"]


def baseline(name):
    if name not in _BASE:
        _BASE[name] = run(name)
    return _BASE[name]


@pytest.mark.parametrize("fill", W.FILLS, ids=[f[0] for f in W.FILLS])
@pytest.mark.parametrize("name", ["keyframe_drops_out", "global_robust"])
def test_stale_arena_contents_change_nothing(name, fill):
    ref, ref_waits = baseline(name)
    _, word, as_next = fill
    nw, _ = W.fill_workspaces(word, as_next)
    assert nw >= 1
    out, waits = run(name)
    for k, (a, b) in enumerate(zip(out, ref)):
        assert a == b, f"{name} after the fill {fill[0]}: output {k} differs from the baseline"
    assert waits == ref_waits
