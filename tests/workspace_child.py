"""Child process of tests/test_gpu_workspace_contents.py: what needs a pool nobody has used yet.  `hook`: the counts
orbm_debug_fill_workspaces reports.  `two`: a pool of exactly two workspaces, both held to the contents test."""
import sys
import threading
import time

import workspace_cases as W
from orb_slam2_e_amd._lib import lib


def same(c, ref, what):
    out, waits, _ = W.run_case(c)
    assert (out, waits) == ref, f"{c.name} {what}: differs from its baseline"


def beside_a_running_thread(body, other="map_poses"):
    """body() while a second thread runs calls without pause"""
    stop = threading.Event()
    errors = []

    def spin():
        try:
            while not stop.is_set():
                W.run_case(W.BY_NAME[other])
        except BaseException as e:
            errors.append(e)
    t = threading.Thread(target=spin)
    t.start()
    try:
        body()
    finally:
        stop.set(); t.join()
    if errors:
        raise errors[0]


def hook():
    assert lib().orbm_debug_fill_workspaces(0, 0, None, None) == -1                   # ORBX_ERR_ARG
    assert W.fill_workspaces(0xFFFFFFFF) == (0, 0), "a fresh process has no workspace and no pooled frame block"
    c = W.BY_NAME["frame_create"]
    ref = W.run_case(c)[:2]
    nw, nb = W.fill_workspaces(0x7FC00000)
    assert nw == 1 and nb >= 1, (nw, nb)                                              # the destroyed frame's block is in its pool
    same(c, ref, "after a fill")
    assert W.fill_workspaces(0, 1) == (nw, nb)
    # a leased workspace is skipped and not counted: the only workspace is inside the other thread's call at some fills (0), free at others (1)
    W.run_case(W.BY_NAME["map_poses"])
    seen = set()

    def fills():
        end = time.monotonic() + 30.0
        while time.monotonic() < end and not seen >= {0, 1}:
            seen.add(W.fill_workspaces(1)[0])
    beside_a_running_thread(fills)
    # Nothing in the ABI blocks inside a lease, so the two states are met by running beside a thread that is inside a call about half
    # of the time: thousands of fills in 30 s.  A count other than 0 or 1 is a defect of the hook; seeing only one of the two means
    # the two threads never interleaved on this machine (a scheduling matter, not a product failure) -- the test still fails, since
    # then it has not shown what it is here to show.
    assert seen <= {0, 1}, f"the fill counted {seen}: the pool holds one workspace"
    assert seen == {0, 1}, f"only {seen} seen in 30 s of fills beside a thread making calls: the threads never interleaved"
    assert W.fill_workspaces(1)[0] == 1


def two():
    cases = [W.BY_NAME[n] for n in sys.argv[2:]]
    refs = {}
    for c in cases:
        out, waits, extra = W.run_case(c)
        if c.check:
            c.check(out, *extra)
        refs[c.name] = (out, waits)
    assert W.fill_workspaces(0)[0] == 1

    def together(a, b, what):
        """a and b at once from two threads: each leases a workspace of its own"""
        errors = []
        gate = threading.Barrier(2)

        def work(c):
            try:
                gate.wait()
                for _ in range(3):
                    same(c, refs[c.name], what)
            except BaseException as e:
                errors.append(e)
        ts = [threading.Thread(target=work, args=(c,)) for c in (a, b)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
        if errors:
            raise errors[0]

    for _ in range(50):                                 # (two calls overlap on the first round unless the machine is very busy)
        together(cases[0], cases[1], "when the second workspace is made")
        if W.fill_workspaces(0)[0] == 2:
            break
    for name, word, as_next in W.FILLS:
        assert W.fill_workspaces(word, as_next)[0] == 2
        for k, c in enumerate(cases):
            # alone: the workspace on top of the free list; together: both are out, whichever thread comes first
            same(c, refs[c.name], f"alone after the fill {name}")
            W.fill_workspaces(word, as_next)
            together(c, cases[(k + 1) % len(cases)], f"with two workspaces after the fill {name}")
            W.fill_workspaces(word, as_next)
    assert W.fill_workspaces(0)[0] == 2


if __name__ == "__main__":
    {"hook": hook, "two": two}[sys.argv[1]]()
    print("child ok")
