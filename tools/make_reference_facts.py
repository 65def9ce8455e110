#!/usr/bin/env python3
"""Regenerates tests/golden/reference_facts.json: what tests/test_cpu_reference_constants.py and tests/test_cpu_integration_shells.py
compare this repository against, read out of a checkout of the reference -- its constants and the digest of its rBRIEF table, the
extractor settings of its launch files, the files that read the members the shells leave empty, and the digest of every run of
reference lines that integration/reference.patch rewrites.  Numbers, paths, line numbers and sha256 digests only: no text of the
reference is stored, so the tests run from this repository alone.

usage: python tools/make_reference_facts.py <reference checkout> [out.json]
Re-run it whenever integration/reference.patch or tools/make_reference_patch.py changes."""
import collections
import glob
import hashlib
import json
import os
import re
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from reference_facts import hunk_digests, ints_digest  # noqa: E402


def nocomment(t):
    return re.sub(r"//[^\n]*", " ", re.sub(r"/\*.*?\*/", " ", t, flags=re.S))


def ints(text):
    return [int(v) for v in re.findall(r"-?\d+", nocomment(text))]


def const(text, name):
    m = re.search(r"\b" + name + r"\s*=\s*([-0-9.eE]+)", nocomment(text))
    assert m, name
    return float(m.group(1))


def strip_comments(t):
    t = re.sub(r"/\*.*?\*/", " ", t, flags=re.S)
    return re.sub(r"//[^\n]*", " ", t)


def sources(ref, *dirs):
    for d in dirs:
        for base, _, names in os.walk(os.path.join(ref, d)):
            for n in sorted(names):
                if n.endswith((".cc", ".cpp", ".h", ".hpp")):
                    yield os.path.join(base, n)


def facts(ref):
    rd = lambda p: open(os.path.join(ref, p), errors="replace").read()
    f = {}
    # ---- extractor: the rBRIEF table (ORBextractor.cc bit_pattern_31_) and the patch / border sizes
    src = rd("src/ORBextractor.cc")
    body = src[src.index("bit_pattern_31_[256*4]"):]
    pat = ints(body[body.index("{") + 1: body.index("};")])
    f["rbrief_pattern"] = {"count": len(pat), "sha256": ints_digest(pat)}
    f["extractor_sizes"] = {n: const(src, n) for n in ("PATCH_SIZE", "HALF_PATCH_SIZE", "EDGE_THRESHOLD")}
    # ---- matcher thresholds (ORBmatcher.cc:37-39)
    m = rd("src/ORBmatcher.cc")
    f["matcher"] = {n: const(m, "ORBmatcher::" + n) for n in ("TH_HIGH", "TH_LOW", "HISTO_LENGTH")}
    # ---- the FEM call: Optimizer.cc builds FEA2(id, E, nu, h, fg, ...); FEA2.cc imposes the encastre with Klarge
    opt = nocomment(rd("src/Optimizer.cc"))
    c = re.search(r"FEA2\s+fea2\(\s*pFrame->mnId\s*,\s*([-0-9.eE]+)\s*,\s*([-0-9.eE]+)\s*,\s*([-0-9.eE]+)\s*,\s*([-0-9.eE]+)\s*,", opt)
    assert c
    klarge = sorted({float(v) for v in re.findall(r"ImposeDirichletEncastre_K\(\s*nMode\s*,\s*\w+\s*,\s*([-0-9.eE]+)\s*\)",
                                                   nocomment(rd("Thirdparty/g2o/g2o/FEA/src/FEA2.cc")))})
    f["fem_call"] = dict(zip(("E", "nu", "h", "fg"), (float(v) for v in c.groups())), Klarge=klarge)
    # ---- the Levenberg hook (optimization_algorithm_levenberg.cpp) and PoseOptimizationNR's rounds (Optimizer.cc)
    lev = nocomment(rd("Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp"))
    trials = re.search(r"_maxTrialsAfterFailure\s*=[^;]*?(\d+)\s*\)?\s*;", lev)
    f["levenberg"] = {"w_rE": sorted(float(v) for v in re.findall(r"w_rE\s*=\s*([0-9.]+)", lev)),
                      "w_sE": sorted(float(v) for v in re.findall(r"w_sE\s*=\s*([0-9.]+)", lev)),
                      "max_trials_after_failure": float(trials.group(1)) if trials else None}
    fn = opt[opt.index("Optimizer::PoseOptimizationNR"):]
    fn = fn[:fn.index("\nint Optimizer::", 10)] if "\nint Optimizer::" in fn[10:] else fn
    its = re.search(r"its\[4\]\s*=\s*\{([^}]*)\}", fn)
    chi = re.search(r"chi2\[4\]\s*=\s*\{([^}]*)\}", fn)
    f["pose_optimization_nr"] = {"its": ints(its.group(1)) if its else None,
                                 "chi2": sorted({float(v) for v in re.findall(r"[0-9.]+", chi.group(1))}) if chi else None,
                                 "uses_sqrt_5_991": bool(re.search(r"sqrt\(5\.991\)", fn))}
    # ---- the fork's launch files (roslaunch/*.yaml, Examples/*/*.yaml)
    tuples, eltype, inverse = collections.Counter(), collections.Counter(), collections.Counter()
    for y in sorted(glob.glob(os.path.join(ref, "roslaunch", "*.yaml")) + glob.glob(os.path.join(ref, "Examples", "*", "*.yaml"))):
        t = open(y, errors="replace").read()
        g = {k: re.search(r"^ORBextractor\." + k + r":\s*([0-9.]+)", t, re.M) for k in ("nFeatures", "scaleFactor", "nLevels", "iniThFAST", "minThFAST")}
        if all(g.values()):
            tuples[tuple(float(v.group(1)) for v in g.values())] += 1
        e = re.search(r"^RelocParam\.nElType:\s*(\d+)", t, re.M)
        if e: eltype[int(e.group(1))] += 1
        i = re.search(r"^RelocParam\.bUseInverse:\s*(\d+)", t, re.M)
        if i: inverse[int(i.group(1))] += 1
    f["launch_files"] = {"extractor_tuples": [[list(k), n] for k, n in tuples.most_common()],
                         "nElType": [[k, n] for k, n in eltype.most_common()], "bUseInverse": [[k, n] for k, n in inverse.most_common()]}
    # ---- who reads ORBextractor::mvImagePyramid, and FEA2::K / vvf
    readers = {}
    for p in sources(ref, "src", "include", "Examples"):
        for k, line in enumerate(open(p, errors="replace"), 1):
            if "mvImagePyramid" in strip_comments(line):
                readers.setdefault(os.path.relpath(p, ref), []).append(k)
    f["mvImagePyramid_readers"] = readers
    kpat = re.compile(r"(->|\.)\s*(K|vvf)\b\s*(\[|\.size|\.push_back|=)")
    live, commented = [], []
    for p in sources(ref, "src", "include", "Thirdparty/g2o/g2o"):
        rel = os.path.relpath(p, ref)
        if "/FEA/" in rel:
            continue
        raw = open(p, errors="replace").read()
        if kpat.search(raw):
            commented.append(rel)
        if kpat.search(strip_comments(raw)):
            live.append(rel)
    f["FEA2_K_vvf_mentions"] = {"live": live, "anywhere": commented}
    # ---- integration/reference.patch: digest of the reference lines each hunk replaces, and of what the generator writes today
    patch = open(os.path.join(ROOT, "integration", "reference.patch"), "rb").read()
    hunks = []
    for rel, start, n, _ in hunk_digests(patch):
        lines = open(os.path.join(ref, rel), "rb").read().splitlines(keepends=True)
        hunks.append([rel, start, n, hashlib.sha256(b"".join(lines[start - 1:start - 1 + n] if n else [])).hexdigest()])
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import make_reference_patch as mrp
    mrp.REF = ref
    with tempfile.TemporaryDirectory() as tmp:
        argv, sys.argv = sys.argv, ["make_reference_patch.py", os.path.join(tmp, "fresh.patch")]
        try:
            mrp.main()
        finally:
            sys.argv = argv
        fresh = open(os.path.join(tmp, "fresh.patch"), "rb").read()
    f["reference_patch"] = {"hunks": hunks, "generated_sha256": hashlib.sha256(fresh).hexdigest(),
                            "generator_sha256": hashlib.sha256(open(mrp.__file__, "rb").read()).hexdigest()}
    return f


if __name__ == "__main__":
    if len(sys.argv) < 2 or not os.path.isdir(os.path.join(sys.argv[1], "src")):
        raise SystemExit(__doc__)
    out = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "reference_facts.json")
    with open(out, "w") as fh:
        json.dump(facts(os.path.abspath(sys.argv[1])), fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", out)
