"""The reference-side shells of integration/ cannot be compiled here (no OpenCV / PCL / g2o); what CAN be checked is: every C-ABI
function they call is declared in include/*.h with that many arguments and exported by the built library, every C-ABI type or
constant they name exists, and the patch applies cleanly to the reference tree.  What these tests know of the reference tree is
tests/golden/reference_facts.json (tools/make_reference_facts.py): digests of the lines the patch rewrites, and which files read
what."""
import hashlib
import os
import re

from reference_facts import hunk_digests, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHELLS = ["ORBextractor_hip.cc", "ORBmatcher_hip.cc", "FEA2_hip.cc", "Frame_stereo_hip.cc", "hip_frame.h"]
REF = load()


def _strip_comments(t):
    t = re.sub(r"/\*.*?\*/", " ", t, flags=re.S)
    return re.sub(r"//[^\n]*", " ", t)


def _declarations():
    """name -> number of parameters, for every function declared in include/*.h; the headers' text without comments"""
    from orb_slam2_e_amd._lib import HEADERS, prototypes
    decl = {name: len(argtypes) for name, (_, argtypes) in prototypes().items()}
    return decl, "".join(_strip_comments(open(h).read()) for h in HEADERS)


def _calls(src):
    """(name, number of arguments) of every call of a C-ABI function in a shell"""
    src = _strip_comments(src)
    out = []
    for m in re.finditer(r"\b((?:orbx|orbm|fem)_[a-z0-9_]+)\s*\(", src):
        i = m.end(); depth = 1; nargs = 0; seen = False
        while depth:
            c = src[i]
            if c in "([{": depth += 1
            elif c in ")]}": depth -= 1
            elif c == "," and depth == 1: nargs += 1
            elif not c.isspace(): seen = True
            i += 1
        out.append((m.group(1), nargs + 1 if seen else 0))
    return out


def test_shells_call_only_declared_and_exported_entry_points():
    decl, header_text = _declarations()
    from orb_slam2_e_amd._lib import lib
    lib = lib()
    ncalls = 0
    for name in SHELLS:
        src = open(os.path.join(ROOT, "integration", name)).read()
        for fn, nargs in _calls(src):
            if fn not in decl:
                # a type / struct tag (orbm_frame, orbx_keypoint, ...) used in a cast or a constructor-style initialiser
                assert re.search(r"\b%s\b" % fn, header_text), f"{name}: {fn} is not in include/*.h"
                continue
            assert decl[fn] == nargs, f"{name}: {fn} called with {nargs} arguments, declared with {decl[fn]}"
            assert hasattr(lib, fn), f"{fn} is declared but not exported"
            ncalls += 1
        for tok in set(re.findall(r"\b(?:ORBX|ORBM|FEM)_[A-Z0-9_]+\b", _strip_comments(src))):
            assert re.search(r"\b%s\b" % tok, header_text), f"{name}: constant {tok} is not in include/*.h"
    assert ncalls > 30


def test_every_matcher_method_of_the_reference_header_is_defined():
    """include/ORBmatcher.h:41-94: 5 SearchByProjection overloads, 2 SearchByBoW, SearchForInitialization, SearchForTriangulation,
    SearchBySim3, 2 Fuse, DescriptorDistance (+ the protected helpers the header declares)."""
    src = _strip_comments(open(os.path.join(ROOT, "integration", "ORBmatcher_hip.cc")).read())
    count = lambda name: len(re.findall(r"^\w[\w \*]*\bORBmatcher::%s\s*\(" % name, src, re.M))
    assert count("SearchByProjection") == 5 and count("SearchByBoW") == 2 and count("Fuse") == 2
    for one in ("SearchForInitialization", "SearchForTriangulation", "SearchBySim3", "DescriptorDistance", "RadiusByViewingCos",
                "ComputeThreeMaxima", "CheckDistEpipolarLine"):
        assert count(one) == 1, one
    assert len(re.findall(r"^ORBmatcher::ORBmatcher\(", src, re.M)) == 1


def test_patch_applies_to_the_reference_tree():
    """Every hunk finds, at its stated line, exactly the reference lines it expects (context and removed lines: what
    `patch --dry-run` checks, without fuzz), and the committed patch is what the generator produced from that tree."""
    raw = open(os.path.join(ROOT, "integration", "reference.patch"), "rb").read()
    files = re.findall(r"^--- a/(\S+)", raw.decode(), re.M)
    assert len(files) >= 9
    rec = REF["reference_patch"]
    got = hunk_digests(raw)
    assert [h[:3] for h in got] == [tuple(h[:3]) for h in rec["hunks"]], "hunks changed: run tools/make_reference_facts.py"
    for (rel, start, n, digest), want in zip(got, rec["hunks"]):
        assert digest == want[3], f"{rel}:{start}: the patch expects other lines than the reference has there"
    # and the committed patch is what the generator produces from this tree
    gen = open(os.path.join(ROOT, "tools", "make_reference_patch.py"), "rb").read()
    assert hashlib.sha256(gen).hexdigest() == rec["generator_sha256"], "tools/make_reference_patch.py changed: run tools/make_reference_facts.py"
    assert hashlib.sha256(raw).hexdigest() == rec["generated_sha256"], "integration/reference.patch is stale: run tools/make_reference_patch.py"


def test_nobody_but_the_replaced_code_reads_mvImagePyramid():
    """ORBextractor::mvImagePyramid is filled on demand (SyncImagePyramid).  Its readers in the reference tree must
    be ORBextractor.cc itself (replaced) and Frame::ComputeStereoMatches (Frame.cc:527-701, replaced by Frame_stereo_hip.cc) --
    anything else would silently read stale levels."""
    readers = REF["mvImagePyramid_readers"]
    assert set(readers) == {"src/ORBextractor.cc", "src/Frame.cc", "include/ORBextractor.h"}, readers
    assert readers["include/ORBextractor.h"] and all(527 <= k <= 701 for k in readers["src/Frame.cc"]), readers
    shell = open(os.path.join(ROOT, "integration", "Frame_stereo_hip.cc")).read()
    assert "orbx_stereo_match" in shell and "mvImagePyramid" not in _strip_comments(shell)
    assert "SyncImagePyramid" in open(os.path.join(ROOT, "integration", "ORBextractor_hip.cc")).read()
    assert "SyncImagePyramid" in open(os.path.join(ROOT, "integration", "reference.patch")).read()
    assert "SyncImagePyramid" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_nobody_but_the_replaced_code_reads_FEA2_K_or_vvf():
    """FEA2::K / vvf stay empty behind the shell.  Outside FEA2.cc (whose numeric methods are replaced) and the
    abandoned FEA.cc the only mention in the reference is the debug print of g2o's Levenberg hook, and that sits inside a comment."""
    live, commented = REF["FEA2_K_vvf_mentions"]["live"], REF["FEA2_K_vvf_mentions"]["anywhere"]
    assert live == [], live
    assert commented == ["Thirdparty/g2o/g2o/core/optimization_algorithm_levenberg.cpp"], commented
    shell = _strip_comments(open(os.path.join(ROOT, "integration", "FEA2_hip.cc")).read())
    assert not re.search(r"\bK\s*(\[|\.push_back|\.resize)", shell) and "vvf" not in shell     # the shell never fills them
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`FEA2::K` and `FEA2::vvf` stay empty" in doc and "levenberg.cpp:173-181" in doc
