"""Static count of the hand-over path of a game-kernel instance: every block of an outermost loop of the kernel that holds a roll loop,
outside that roll loop (the roll loop: the Depth=2 loop with the most v_mad_u64_u32, with everything nested in it, as tools/isa_mix.py
takes it; that tool reads only Depth=2 loops, this one needs the whole loop tree, so the block parsing is its own).  The two-seat tournament instance holds the loop nest twice (flat / general hand-over): one line per copy, the flat one first.
usage: python tools/isa_handover_path.py [file.s] [symbol regex]
Without a file the device code is compiled to assembly first (~100 s; tools/isa_mix.py leaves the same file in tools/ab/).  Counted: VALU
(lane-crossing reads and writes left out, as in isa_mix.py), v_mov, branches, scalar loads, waits, 64-bit multiply-adds and adds, global
loads / stores, LDS instructions, 24-bit multiplies, selects; the kernel's VGPRs, scratch and occupancy from its resource comment."""
import re, subprocess, sys
from collections import Counter
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
CONFIG2 = r"fk_play_kernelILi768ELb1ELi6ELj49152ELb0ELb0ELi2EEE"


def kernel_body(path, want):
    name, body, found = None, [], None
    for line in open(path):
        if re.match(r"^_ZN\w+:", line):
            name, body = line.split(":")[0], []
        elif name is not None:
            body.append(line.rstrip("\n"))
            if "s_endpgm" in line:
                if re.search(want, name):
                    found = (name, body)
                name = None
    return found


def basic_blocks(body):
    fn = next(re.match(r"\.LBB(\d+)_", l).group(1) for l in body if l.startswith(".LBB"))
    blocks, bn, ann, ins = [], None, "", []
    for l in body:
        m = re.match(r"^\.L(BB\d+_\d+):", l) or re.match(r"^; %bb\.(\d+):", l)
        if m:
            if bn:
                blocks.append((bn, ann, ins))
            bn = m.group(1) if m.group(1).startswith("BB") else f"BB{fn}_{m.group(1)}"
            ann, ins = l, []
        elif bn and l.lstrip().startswith(";") and not ins:
            ann += " " + l
        elif bn and l.startswith("\t") and not l.strip().startswith((";", ".")):
            ins.append(l.split()[0])
    if bn:
        blocks.append((bn, ann, ins))
    return blocks


def valu(ops):
    return sum(c for o, c in ops.items() if o.startswith("v_") and not o.startswith(("v_readlane", "v_readfirstlane", "v_writelane")))


def main():
    asm = Path(sys.argv[1]) if len(sys.argv) > 1 else ROOT / "tools" / "ab" / "farkle_hip_gfx950.s"
    want = sys.argv[2] if len(sys.argv) > 2 else CONFIG2
    if len(sys.argv) <= 1:
        asm.parent.mkdir(exist_ok=True)
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-I", str(ROOT / "include"), "-S", "--cuda-device-only", "-o", str(asm),
                        str(ROOT / "farkle_ii_amd" / "csrc" / "farkle_hip.hip")], check=True, capture_output=True)
    found = kernel_body(asm, want)
    if found is None:
        raise SystemExit(f"no kernel whose symbol matches {want!r} in {asm}")
    name, body = found
    blocks = basic_blocks(body)
    # the loop tree: a block names only its innermost loop's header, a header names its parent loops
    parents = {b[0]: re.findall(r"Parent Loop (BB\d+_\d+)", b[1]) for b in blocks if "Loop Header: Depth=" in b[1]}

    def header_of(b):
        if "Loop Header: Depth=" in b[1]:
            return b[0]
        m = re.search(r"Header=(BB\d+_\d+)", b[1])
        return m.group(1) if m else None

    def in_loop(b, h):
        hb = header_of(b)
        return hb is not None and (hb == h or h in parents.get(hb, []))

    print(name)
    for h, a, _ in blocks:
        if "Loop Header: Depth=1" not in a:
            continue
        members = [b for b in blocks if in_loop(b, h)]
        roll, best = set(), -1
        for ih in (b[0] for b in members if "Loop Header: Depth=2" in b[1]):
            inner = [b for b in members if in_loop(b, ih)]
            n = sum(1 for b in inner for o in b[2] if o == "v_mad_u64_u32")
            if n > best:
                best, roll = n, set(b[0] for b in inner)
        if best < 3:
            continue  # not a copy of the game loop nest (the tally's clearing and flushing loops)
        ops = Counter(o for b in members if b[0] not in roll for o in b[2])
        rops = Counter(o for b in members if b[0] in roll for o in b[2])
        g = lambda p: sum(c for o, c in ops.items() if o.startswith(p))
        print(f"{h}: path VALU {valu(ops)} v_mov {g('v_mov')} branches {g('s_cbranch') + g('s_branch')} s_load {g('s_load')} s_waitcnt {g('s_waitcnt')} "
              f"mad64 {g('v_mad_u64')} lshl_add64 {g('v_lshl_add_u64')} global_load {g('global_load')} global_store {g('global_store')} LDS {g('ds_')} "
              f"mul24 {g('v_mul_u32_u24')} mulhi24 {g('v_mul_hi_u32_u24')} cndmask {g('v_cndmask')} | roll loop with its nested loops VALU {valu(rops)}")
    txt = open(asm).read()
    tail = txt[txt.index(name + ":"):]
    print("  ".join(key + " " + re.search(r"; " + key + r": (\d+)", tail).group(1) for key in ("NumVgprs", "ScratchSize", "Occupancy")))


if __name__ == "__main__":
    main()
