"""Every place where a matcher-side entry point leases a pooled workspace has a case in tests/workspace_cases.py (run on the GPU by
tests/test_gpu_workspace_contents.py): the StagedCall / WorkspaceLease declarations of csrc/ are counted per file and compared
with the table's SITES; a new lease site without a case fails here, without a GPU.  Also the ABI surface of the two debug entries
those tests use."""
import ctypes as C
import os
import re
import subprocess

import workspace_cases as W
from orb_slam2_e_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "orb_slam2_e_amd", "csrc")
DECL = re.compile(r"^\s*(?:orbm_detail::)?(?:StagedCall|WorkspaceLease)\s+\w+\s*;", re.M)


def declarations():
    """file -> number of StagedCall / WorkspaceLease variables (or members) it declares"""
    out = {}
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".h", ".inc")):
            with open(os.path.join(CSRC, f)) as fh:
                n = len(DECL.findall(fh.read()))
            if n:
                out[f] = n
    return out


def test_the_pattern_finds_a_declaration_and_nothing_else():
    text = "    StagedCall sc;\n        orbm_detail::WorkspaceLease lease;\nint f(const orbm_kfdb *db, StagedCall &sc, size_t o);\n" \
           "struct WorkspaceLease {\n    WorkspaceLease() : w(workspace_acquire()) {}\n// a StagedCall sc; in a comment\n"
    assert len(DECL.findall(text)) == 2


def test_every_lease_site_is_in_the_table():
    found = declarations()
    assert found == {f: len(names) for f, names in W.SITES.items()}, "a lease site was added or removed: update tests/workspace_cases.py (SITES and a case)"
    assert sum(n for f, n in found.items() if f.endswith(".hip")) == 33


def test_every_site_in_the_table_has_a_case():
    sites = {f"{f}/{name}" for f, names in W.SITES.items() for name in names}
    assert len(sites) == sum(len(v) for v in W.SITES.values())
    assert W.tagged_sites() <= sites
    assert sites - W.tagged_sites() == W.NOT_A_CALL


def test_every_borrowed_helper_exists():
    """the table's lazy imports from the units' test modules, made here: a renamed helper fails without a GPU"""
    import importlib
    with open(W.__file__) as f:
        src = f.read()
    used = {}
    for mod, names in re.findall(r"^\s*from (test_\w+) import (.+)$", src, re.M):
        used.setdefault(mod, set()).update(n.split(" as ")[0].strip() for n in names.split(","))
    assert used == {m: set(v) for m, v in W.HELPERS.items()}
    for mod, names in W.HELPERS.items():
        m = importlib.import_module(mod)
        for n in names:
            assert hasattr(m, n), f"{mod}.{n}"
    for c in W.CASES:
        assert c.check is not None, f"{c.name}: no comparison with its unit's oracle or restatement"


def test_the_search_family_has_a_case_per_path():
    """run_sequential: explicit lists, strided windows, the exact path, SearchForInitialization, the forced sequential resolver, the
    chained tracking calls"""
    names = {c.name for c in W.CASES if "orbm_search.hip/run_sequential" in c.sites}
    assert {"search_by_bow", "projection_windows", "projection_windows_overflow", "search_for_initialization", "projection_windows_sequential",
            "search_by_bow_sequential", "track_motion_model", "track_local_map"} <= names
    assert [f[0] for f in W.FILLS] == ["zero", "one", "next_generation", "nan", "minus_one"]
    assert [(f[1], f[2]) for f in W.FILLS] == [(0, 0), (1, 0), (0, 1), (0x7FC00000, 0), (0xFFFFFFFF, 0)]


def test_abi_of_the_debug_entries():
    so = _lib.build()
    protos = _lib.prototypes()
    assert protos["orbm_debug_fill_workspaces"] == (C.c_int, [C.c_uint32, C.c_int, C.c_void_p, C.c_void_p])
    assert protos["orbm_debug_last_search_waits"] == (C.c_int, [])
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    assert " T orbm_debug_fill_workspaces\n" in out and " T orbm_debug_last_search_waits\n" in out
    L = _lib.lib()
    assert L.orbx_abi_version() == 136                                          # additions only
    nw, nb = C.c_int(-7), C.c_int(-7)
    assert L.orbm_debug_fill_workspaces(0, 0, None, C.byref(nb)) == -1 and L.orbm_debug_fill_workspaces(0, 0, C.byref(nw), None) == -1
    assert (nw.value, nb.value) == (-7, -7)                                     # a refused call writes nothing
    rc = L.orbm_debug_fill_workspaces(0, 0, C.byref(nw), C.byref(nb))
    assert rc in (0, -2) and (rc == 0 or (nw.value, nb.value) == (0, 0))        # no device: ORBX_ERR_NO_DEVICE, counts 0
    assert L.orbm_debug_last_search_waits() >= 0
