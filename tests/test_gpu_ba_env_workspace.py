"""orbm_global_bundle_adjustment_env's bytes and host waits do not depend on what its pooled workspace held before ("What a
call may assume about its workspace"): the lease site the three entries of orbm_ba.hip share, on the envelope path, under the fills
of tests/workspace_cases.py.  What the envelope path adds is written before it is read: the live tiles by the fill on the stream and
k_ba_schur_env each trial, the running dots W by the panel that starts them, the plan image by the upload and, for the second round,
by the upload of the re-planned image (e70_drop: a keyframe leaves, the rows shift), xp and the ok word by the solve.  No tolerance:
the comparator is the same call in the same process."""
import pytest

import ba_env_scenes as ES
import workspace_cases as W
from orb_slam2_e_amd import bundle
from test_gpu_ba_large import image

pytestmark = pytest.mark.gpu
NAMES = ("e70_drop", "e65_loop")
_BASE = {}


def run(name):
    _, g, opt = ES.scene(name)
    r = bundle.run_global_env(g, opt, want_stats=True)
    return image(r), r["waits"]


def baseline(name):
    if name not in _BASE:
        _BASE[name] = run(name)
    return _BASE[name]


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("fill", W.FILLS, ids=[f[0] for f in W.FILLS])
def test_stale_arena_contents_change_nothing(fill, name):
    ref, ref_waits = baseline(name)
    _, word, as_next = fill
    nw, _ = W.fill_workspaces(word, as_next)
    assert nw >= 1
    out, waits = run(name)
    for k, (a, b) in enumerate(zip(out, ref)):
        assert a == b, f"{name} after the fill {fill[0]}: output {k} differs from the baseline"
    assert waits == ref_waits
