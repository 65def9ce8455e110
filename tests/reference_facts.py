"""tests/golden/reference_facts.json (written by tools/make_reference_facts.py from a checkout of the reference) and the two
digests it is made of, shared by the generator and the tests that read it."""
import hashlib
import json
import os
import re

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_facts.json")


def load():
    with open(GOLDEN) as f:
        return json.load(f)


def ints_digest(values):
    """sha256 of a table of integers, written as decimal numbers joined by commas."""
    return hashlib.sha256(",".join(str(int(v)) for v in values).encode()).hexdigest()


def hunk_digests(patch):
    """(file, old start, old length, sha256 of the old side) of every hunk of a unified diff (bytes): the lines the hunk expects
    to find in the file it is applied to -- its context and removed lines, with their line ends."""
    out = []
    rel, old, want, start = None, [], 0, 0
    lines = patch.splitlines(keepends=True)
    for k, line in enumerate(lines):
        if want:
            if line.startswith((b" ", b"-")):
                body = line[1:]
                if k + 1 < len(lines) and lines[k + 1].startswith(b"\\"):     # "\ No newline at end of file"
                    body = body.rstrip(b"\r\n")
                old.append(body)
                want -= 1
                if not want:
                    out.append((rel, start, len(old), hashlib.sha256(b"".join(old)).hexdigest()))
            continue
        m = re.match(rb"^--- a/(\S+)", line)
        if m:
            rel = m.group(1).decode()
            continue
        m = re.match(rb"^@@ -(\d+)(?:,(\d+))? \+\d+(?:,\d+)? @@", line)
        if m:
            start, want, old = int(m.group(1)), int(m.group(2) or 1), []
            if not want:
                out.append((rel, start, 0, hashlib.sha256(b"").hexdigest()))
    return out
