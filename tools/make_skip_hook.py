#!/usr/bin/env python3
"""Regenerates tools/skip_hook.patch (the ORBX_SKIP development hook of tools/saturated.sh) against the current sources:
applies the edits in place, writes `git diff` of csrc/ to the patch file and restores the sources.  Run from the repo root
with a clean orb_slam2_e_amd/csrc."""
import subprocess, sys

if subprocess.run(["git", "diff", "--quiet", "--", "orb_slam2_e_amd/csrc"]).returncode != 0:
    sys.exit("orb_slam2_e_amd/csrc has uncommitted changes: this script restores it from git when it is done -- commit or stash first")

def edit(path, pairs):
    s = open(path).read()
    for old, new in pairs:
        assert s.count(old) == 1, (path, old[:80], s.count(old))
        s = s.replace(old, new)
    open(path, "w").write(s)

hook = ('    static int skipmask = getenv("ORBX_SKIP") ? atoi(getenv("ORBX_SKIP")) : 0; static int ncalls = 0; ++ncalls;\n')
# the six launch calls of orbx_extract_batch, one bit each (a skipped stage's profiler bracket goes with it)
stages = [("launch_level0(ex, d_img, stride, frame_stride, batch, st);", 1), ("launch_pyramid(ex, batch, st);", 2), ("launch_fast(ex, batch, st);", 4),
          ("launch_octree(ex, batch, st);", 8), ("launch_blur(ex, batch, st);", 16), ("launch_describe(ex, batch, st);", 32)]
edit("orb_slam2_e_amd/csrc/orbx_extract.hip",
     [("    " + stages[0][0] + "\n", hook + "    const int SK = ncalls < 8 ? 0 : skipmask;\n    " + stages[0][0] + "\n")] +
     [("    " + call + "\n", "    if (!(SK & %d)) " % bit + call + "\n") for call, bit in stages])
edit("orb_slam2_e_amd/csrc/orbm_match.hip", [
    ("                              int th, float nnratio, int *best, int *second, int *idx, int *match12, int *nmatch)\n{\n",
     "                              int th, float nnratio, int *best, int *second, int *idx, int *match12, int *nmatch)\n{\n" + hook +
     "    if (ncalls >= 8 && (skipmask & 64)) return;\n"),
])
open("tools/skip_hook.patch", "w").write(subprocess.check_output(["git", "diff", "--", "orb_slam2_e_amd/csrc"], text=True))
if "--keep" not in sys.argv:
    subprocess.check_call(["git", "checkout", "--", "orb_slam2_e_amd/csrc"])
print("tools/skip_hook.patch written")
