"""Compare two device-side assembly listings of farkle_hip.hip symbol by symbol.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S -o A.s farkle_ii_amd/csrc/farkle_hip.hip   (at each commit)
    python tools/compare_device_code.py A.s B.s [--allow REGEX]

A listing is split at its symbols (`name:` at column 0 up to `.Lfunc_end`, which takes a kernel's descriptor in, or up to `.size` for
data) and at the kernels' metadata entries; a body is its text with local-label, basic-block and function ordinals replaced by their
order of appearance, and is otherwise opaque.  Prints the number of bodies, the symbols present on one side only, the differing bodies,
and how many `fk_play` function names both sides share.  Exit status 1 if a symbol is missing or a body outside --allow differs."""
from __future__ import annotations

import argparse
import re
import sys

ORDINAL = re.compile(r"\.L(?:BB|func_begin|func_end|tmp|JTI)?[0-9_]+|%bb\.[0-9]+|@function ordinal [0-9]+")


def bodies(path: str) -> dict[str, str]:
    out: dict[str, list[str]] = {}
    name = None
    text, _, metadata = open(path, errors="replace").read().partition("\t.amdgpu_metadata\n")
    for entry in metadata.split("  - .agpr_count:")[1:]:  # one metadata entry per kernel
        out["metadata " + re.search(r"\.name:\s+(\S+)", entry).group(1)] = [entry]
    for line in text.splitlines(keepends=True):
        m = re.match(r"([A-Za-z_][\w$.]*):", line)
        if m and name is None and not line.startswith((".L", "__hip_cuid_")):  # (the unit id is a hash of the source)
            name = m.group(1)
            out[name] = []
        if name is not None:
            out[name].append(line)
            if line.startswith((".Lfunc_end", "\t.size")):
                name = None
    norm = {}
    for k, lines in out.items():
        seen: dict[str, str] = {}
        norm[k] = ORDINAL.sub(lambda m: seen.setdefault(m.group(0), f"<{len(seen)}>"), "".join(lines))
    return norm


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("a")
    ap.add_argument("b")
    ap.add_argument("--allow", default=None, help="symbols whose bodies may differ")
    args = ap.parse_args()
    a, b = bodies(args.a), bodies(args.b)
    only = sorted(set(a) ^ set(b))
    diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
    bad = [k for k in diff if not (args.allow and re.search(args.allow, k))]
    play = lambda d: {k for k in d if "fk_play" in k and " " not in k}
    print(f"{len(a)} / {len(b)} bodies, {len(only)} symbols on one side only, {len(diff)} differing bodies ({len(bad)} not allowed), "
          f"{len(play(a) & play(b))} of {len(play(a))} fk_play names shared")
    for k in only:
        print("one side only:", k)
    for k in diff:
        print("differs:", k)
    return 1 if only or bad else 0


if __name__ == "__main__":
    sys.exit(main())
