"""The Python side of the C ABI against include/*.h: every declared function carries its header prototype (orb_slam2_e_amd/_lib.py
prototypes()), the library exports exactly the declared functions, and the Python mirrors of the C structs have the C layout
(tests/cxx/abi_layout.c, compiled against the headers)."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from orb_slam2_e_amd import _lib
from orb_slam2_e_amd.extractor import KP_DTYPE, _ExtractPlan, _Params
from orb_slam2_e_amd.fem import _PlanInfo
from orb_slam2_e_amd.matcher import ORBmatcher, _CPoints, _CView
from orb_slam2_e_amd.pose import PoseCamera, PoseStats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# exported without a declaration on purpose: development aids of fem.hip that tools/fem_xcd_debug.py and tools/fem_xcd_phases.py call
UNDECLARED_EXPORTS = {"fem_debug_xcd", "fem_debug_xcd_timing"}

MIRRORS = {"orbx_keypoint": KP_DTYPE, "orbx_params": _Params, "orbx_plan_info": _ExtractPlan, "fem_plan_info": _PlanInfo,
           "orbm_window_query": ORBmatcher.WQ_DTYPE, "orbm_camera": ORBmatcher.CAM_DTYPE, "orbm_projected_point": ORBmatcher.PROJ_DTYPE,
           "orbm_points": _CPoints, "orbm_view": _CView, "orbm_pose_camera": PoseCamera, "orbm_pose_stats": PoseStats}


@pytest.fixture(scope="module")
def so():
    """The product library brought up to date with include/*.h by its makefile: a header prototype that no longer matches its
    definition does not compile."""
    return _lib.build()


def test_every_declared_function_carries_its_header_prototype(so):
    protos = _lib.prototypes()
    assert len(protos) > 100
    # the mapping itself, on declarations that use each kind of parameter
    assert protos["orbx_last_error"] == (C.c_char_p, [])
    assert protos["orbx_abi_version"] == (C.c_int, [])
    assert protos["fem_create"] == (C.c_int, [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_uint, C.c_float, C.c_float,
                                              C.c_void_p])
    assert protos["fem_cg"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_void_p, C.c_void_p])
    assert protos["orbx_extract_batch"] == (C.c_int, [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_size_t, C.c_int,
                                                      C.c_void_p])
    assert protos["fem_profile_read"][1] == [C.c_void_p, C.c_int] + [C.c_void_p] * 4          # const char **, int64_t *
    L = _lib.lib()
    for name, (restype, argtypes) in protos.items():
        fn = getattr(L, name)
        assert fn.restype is restype and list(fn.argtypes) == argtypes, name
    assert L.orbx_abi_version() == 136


def test_declared_types_refuse_a_wrong_python_value(so):
    """What an untyped call passed on silently: a float into an int parameter, a ctypes float into a double one."""
    L = _lib.lib()
    with pytest.raises(C.ArgumentError):
        L.orbm_set_allpairs_kernel(1.0)
    with pytest.raises(C.ArgumentError):
        L.fem_cg(None, None, None, 1, C.c_float(0.5), None, None)


def test_a_parameter_type_outside_the_table_raises(tmp_path, monkeypatch):
    for decl in ("int orbx_x(long n);", "int orbx_x(int64_t n);", "int orbx_x(float v[3]);", "float orbx_x(void);", "int orbx_x(int);"):
        h = tmp_path / "x.h"
        h.write_text("/* a header */\n#include <stdint.h>\n" + decl + "\n")
        monkeypatch.setattr(_lib, "HEADERS", (str(h),))
        with pytest.raises(RuntimeError, match="orbx_x"):
            _lib.prototypes()


def test_a_declared_function_the_library_lacks_fails_the_load(tmp_path, monkeypatch, so):
    h = tmp_path / "x.h"
    h.write_text(open(_lib.HEADERS[0]).read() + "\nint orbx_not_exported(void);\n")
    monkeypatch.setattr(_lib, "HEADERS", (str(h),))
    monkeypatch.setattr(_lib, "_LIB", None)
    with pytest.raises(RuntimeError, match="orbx_not_exported"):
        _lib.lib()


def test_library_builds_and_exports_exactly_the_declared_functions(so):
    out = subprocess.check_output(["nm", "-D", "--defined-only", so]).decode()
    exported = set(re.findall(r"^\S+ \S ((?:orbx|orbm|fem)_\w+)$", out, re.M))
    declared = set(_lib.prototypes())
    assert not declared - exported, "declared in include/*.h but not exported"
    assert exported - declared == UNDECLARED_EXPORTS


@pytest.fixture(scope="module")
def c_layout(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("abi") / "abi_layout")
    subprocess.check_call(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "cxx", "abi_layout.c"), "-o", exe])
    layout = {}
    for line in subprocess.check_output([exe]).decode().splitlines():
        kind, struct, *rest = line.split()
        if kind == "struct":
            layout[struct] = (int(rest[0]), [])
        else:
            layout[struct][1].append((rest[0], int(rest[1]), int(rest[2])))
    return layout


def _py_layout(m):
    """(size, [(field, offset, width)]) of a numpy dtype or a ctypes Structure"""
    if isinstance(m, np.dtype):
        return m.itemsize, [(n, m.fields[n][1], m.fields[n][0].itemsize) for n in m.names]
    return C.sizeof(m), [(f[0], getattr(m, f[0]).offset, getattr(m, f[0]).size) for f in m._fields_]


def test_the_layout_program_covers_every_mirror(c_layout):
    assert set(c_layout) == set(MIRRORS)


@pytest.mark.parametrize("struct", sorted(MIRRORS))
def test_python_mirror_has_the_c_layout(struct, c_layout):
    size, fields = c_layout[struct]
    psize, pfields = _py_layout(MIRRORS[struct])
    assert psize == size, f"{struct}: {psize} bytes in Python, {size} in C"
    assert len(pfields) == len(fields), f"{struct}: fields {[f[0] for f in pfields]} in Python, {[f[0] for f in fields]} in C"
    for (pn, po, pw), (cn, co, cw) in zip(pfields, fields):
        assert (po, pw) == (co, cw), f"{struct}.{cn}: offset {co} width {cw} in C; Python field {pn}: offset {po} width {pw}"
