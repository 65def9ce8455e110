"""Builds a C restatement under tests/ into a shared object for ctypes (test infrastructure: never part of the product)."""
import hashlib
import os
import subprocess
import tempfile


def build(src, includes=(), flags=("-O2",)):
    """The shared object of the C file `src` compiled with gcc and `flags` (always -ffp-contract=off -fno-fast-math -std=c99), built
    on first use into a per-user cache directory and moved into place atomically.  `includes`: the files `src` includes; the
    cache tag covers them, the source and the flags, so editing any of them builds a new object."""
    h = hashlib.sha256(" ".join(flags).encode())
    for path in (src, *includes):
        h.update(b"\0" + open(path, "rb").read())
    stem = os.path.splitext(os.path.basename(src))[0]
    d = os.path.join(tempfile.gettempdir(), f"orbslam_{stem}_{os.getuid()}")
    os.makedirs(d, exist_ok=True)
    so = os.path.join(d, f"{stem}_{h.hexdigest()[:16]}.so")
    if not os.path.exists(so):
        tmp = so + f".{os.getpid()}.tmp"
        subprocess.check_call(["gcc", *flags, "-ffp-contract=off", "-fno-fast-math", "-std=c99", "-shared", "-fPIC", "-o", tmp, src, "-lm"])
        os.replace(tmp, so)
    return so
