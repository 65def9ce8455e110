"""A call's bytes and its host-wait count do not depend on what its pooled workspace held before ("What a call may
assume about its workspace").  Every matcher-side entry point carves its arrays out of one process-wide pool of workspaces
(orbm_detail::Workspace: a device arena, a pinned arena, an entries buffer), always from offset 0, so the last call's data -- of
another entry point, another layout, other types -- lies under the next call's arrays; a frame is built on a recycled block.
orbm_debug_fill_workspaces sets those contents; tests/workspace_cases.py holds one case per lease site.

There is no tolerance anywhere: the comparator is the same call in the same process, and every unit asserts on its own that its
call is deterministic.  The fills are values arenas do hold after other calls: zeros (a fresh arena), 1, the generation number the
next call's flags carry, a float NaN (a large int), -1 (the "none" marker)."""
import os
import subprocess
import sys

import pytest

import workspace_cases as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_BASE = {}


def baseline(c):
    """the case once on whatever the arena held, held to its oracle where the case has one; shared by every test, never changed"""
    if c.name not in _BASE:
        out, waits, extra = W.run_case(c)
        if c.check:
            c.check(out, *extra)
        _BASE[c.name] = (out, waits)
    return _BASE[c.name]


def same_as_baseline(c, what):
    out, waits, _ = W.run_case(c)
    ref, ref_waits = baseline(c)
    assert len(out) == len(ref), f"{c.name} {what}: {len(out)} outputs, {len(ref)} in the baseline"
    for k, (a, b) in enumerate(zip(out, ref)):
        assert a == b, f"{c.name} {what}: output {k} differs from the baseline"
    assert waits == ref_waits, f"{c.name} {what}: {waits} host waits, {ref_waits} in the baseline"
    return waits


# ---------------------------------------------------------------------------------------------------------------- contents

@pytest.mark.parametrize("fill", W.FILLS, ids=[f[0] for f in W.FILLS])
@pytest.mark.parametrize("c", W.CASES, ids=repr)
def test_contents(c, fill):
    baseline(c)
    _, word, as_next = fill
    nw, _ = W.fill_workspaces(word, as_next)
    assert nw >= 1
    same_as_baseline(c, f"after the fill {fill[0]}")


# --------------------------------------------------------------------------------------------------------- the named defect

@pytest.mark.parametrize("name", sorted(W.EXPECTED_WAITS))
def test_a_stale_generation_number_is_no_flag(name):
    """"A list outgrew its region" is raised by writing the call's generation number and read by comparing with it; the word used to
    lie in device memory that nothing wrote before.  With every word of the arena equal to that number: the searches whose lists fit
    and the chained tracking calls still wait once, and the scene whose lists do overflow still repeats (strided attempt, sizing
    wait of the exact lists, exact attempt)."""
    c = W.BY_NAME[name]
    assert baseline(c)[1] == W.EXPECTED_WAITS[name]
    W.fill_workspaces(0, 1)
    assert same_as_baseline(c, "after the next-generation fill") == W.EXPECTED_WAITS[name]


# ------------------------------------------------------------------------------------------------------------ natural dirt

def test_every_call_behind_calls_of_other_units():
    """No hook: every case behind a larger call of ANOTHER unit, then behind a smaller one -- what a process does all day."""
    unit = lambda c: c.sites[0].split("/")[0]
    large = [c for c in W.CASES if c.weight > 1]
    small = [c for c in W.CASES if c.weight == 1]
    for c in W.CASES:
        baseline(c)
    for k, c in enumerate(W.CASES):
        for pool, size in ((large, "larger"), (small, "smaller")):
            others = [o for o in pool if unit(o) != unit(c)]
            before = others[k % len(others)]
            same_as_baseline(before, f"in front of {c.name}")
            same_as_baseline(c, f"behind the {size} call {before.name}")


# ------------------------------------------------------------------------------------------- what needs a fresh process

TWO = ("projection_windows", "track_local_map", "kfdb_query")


def _child(*args):
    env = dict(os.environ, PYTHONPATH=os.pathsep.join([ROOT] + [p for p in os.environ.get("PYTHONPATH", "").split(os.pathsep) if p]))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "workspace_child.py"), *args], capture_output=True, text=True, env=env,
                       timeout=600)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


def test_two_workspaces():
    """Two calls at once from two threads lease two workspaces: the fill then reports 2, and three cases pass the contents test on
    both (alone: the one on top of the free list; two at once: both).  A child process, because this one's pool holds as many
    workspaces as the most concurrent test before it needed."""
    _child("two", *TWO)


def test_the_hook_in_a_fresh_process():
    """0 workspaces and 0 frame blocks before any call, 1 and >= 1 after one, a leased workspace skipped and not counted."""
    _child("hook")
