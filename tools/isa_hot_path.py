"""The roll loop's hot path of a game-kernel instance, from the compiler's assembly (hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S).
usage: python tools/isa_hot_path.py <file.s> [symbol regex] [--take LABEL[,LABEL...]] [--fall LABEL[,LABEL...]] [--blocks]

The roll loop is the loop at Depth 2 or deeper with the most v_mad_u64_u32, the innermost of several that hold the same draws (tools/isa_mix.py
takes it the same way; since round 14 the block instance's roll loop sits inside a Depth=2 loop of its full hand-over test); the two-seat
tournament instance holds the loop nest twice (flat / general hand-over): one report per copy, the flat one first.  The walk starts at
the loop's header and ends where it comes back to it.  At a conditional branch it decides like this, and prints every decision:
  * a branch to the loop's header is the back branch: taken;
  * a forward branch on the exec mask (s_cbranch_execz / execnz) is taken when the blocks it jumps over hold a nested loop or a global
    atomic (the Lemire replay, the `raise` block: rare blocks left in line), otherwise not (a draw region, the store, the change of owner:
    some lane needs them in nearly every trip);
  * a branch that leaves the loop is not taken;
  * any other conditional branch is NOT taken, the fall-through, unless the block it ends is named in --take (--fall: the opposite,
    for one of the rules above).  A scalar branch's direction is not in the file: the reader names the ones the hot trip takes.
An s_branch is always taken.  Counted along the path: vector, scalar (ALU and moves; s_nop, s_waitcnt, branches and scalar loads apart),
s_nop, branches whose target is not the next block in the file (what the instruction fetch pays), branches fallen through, waits, LDS,
vector memory, scalar memory.  It reads; it is not a test."""
import argparse
import re
from collections import Counter

CONFIG2 = r"fk_play_kernelILi768ELb1ELi6ELj49152ELb0ELb0ELi2EEE"


def kernel_body(path, want):
    name, body, found = None, [], None
    for line in open(path):
        if re.match(r"^_ZN\w+:", line):
            name, body = line.split(":")[0], []
        elif name is not None:
            body.append(line.rstrip("\n"))
            if "s_endpgm" in line:
                if found is None and re.search(want, name):
                    found = (name, body)
                name = None
    return found


def basic_blocks(body):
    """[(label, annotation, [(opcode, operands)])] in the file's order"""
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
            t = l.split(";")[0].split(None, 1)
            ins.append((t[0], t[1].strip() if len(t) > 1 else ""))
    if bn:
        blocks.append((bn, ann, ins))
    return blocks


def classify(op):
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op == "s_nop":
        return "s_nop"
    if op.startswith("s_waitcnt"):
        return "wait"
    if op.startswith(("s_load", "s_buffer_load")):
        return "scalar memory"
    if op.startswith("s_"):
        return "scalar"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "vector memory"
    if op.startswith("v_"):
        return "vector"
    return "other"


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("asm")
    ap.add_argument("symbol", nargs="?", default=CONFIG2)
    ap.add_argument("--take", default="", help="blocks whose closing conditional branch the hot trip takes")
    ap.add_argument("--fall", default="", help="blocks whose closing conditional branch the hot trip falls through, against the rules")
    ap.add_argument("--blocks", action="store_true", help="print the instructions of every block on the path")
    args = ap.parse_args()
    take, fall = set(filter(None, args.take.split(","))), set(filter(None, args.fall.split(",")))
    found = kernel_body(args.asm, args.symbol)
    if found is None:
        raise SystemExit(f"no kernel whose symbol matches {args.symbol!r} in {args.asm}")
    name, body = found
    blocks = basic_blocks(body)
    index = {b[0]: i for i, b in enumerate(blocks)}
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
    for outer, a, _ in blocks:
        if "Loop Header: Depth=1" not in a:
            continue
        members = [b for b in blocks if in_loop(b, outer)]
        head, best = None, -1
        for ih in (b[0] for b in members if re.search(r"Loop Header: Depth=[2-9]", b[1])):  # in the file's order: of two nested loops that
            n = sum(1 for b in members if in_loop(b, ih) for o, _ in b[2] if o == "v_mad_u64_u32")  # hold the same draws, the inner one
            if n >= best and n > 0:
                best, head = n, ih
        if best < 3:
            continue  # not a copy of the game loop nest
        loop = set(b[0] for b in members if in_loop(b, head))
        static = Counter(classify(o) for b in members if b[0] in loop for o, _ in b[2])
        print(f"\nouter loop {outer}, roll loop {head}: {len(loop)} blocks; static, rare blocks included: " + ", ".join(f"{k} {v}" for k, v in sorted(static.items())))

        def rare(i_from, i_to):  # the blocks a forward branch jumps over
            over = blocks[i_from + 1:i_to]
            return any("Loop Header" in b[1] for b in over) or any(o.startswith("global_atomic") for b in over for o, _ in b[2])

        counts, path, notes, seen = Counter(), [], [], set()
        i, done = index[head], False
        while not done:
            label, _, ins = blocks[i]
            if label in seen:
                notes.append(f"  {label}: reached a second time before the header: the walk stops here (name a branch with --take)")
                break
            seen.add(label)
            path.append(label)
            if args.blocks:
                print(f"  {label}:")
            nxt = i + 1
            for op, arg in ins:
                if args.blocks:
                    print(f"      {op} {arg}")
                c = classify(op)
                if c != "branch":
                    counts[c] += 1
                    continue
                target = arg.strip().lstrip(".L")
                j = index.get(target)
                if op == "s_branch":
                    taken, why = True, "always"
                elif label in take:
                    taken, why = True, "--take"
                elif label in fall:
                    taken, why = False, "--fall"
                elif target == head or target in seen:  # (a rotated loop's back branch may aim behind the header's preamble)
                    taken, why = True, "the back branch"
                elif target not in loop:
                    taken, why = False, "leaves the loop"
                elif op in ("s_cbranch_execz", "s_cbranch_execnz") and j is not None and j > i:
                    taken = rare(i, j)
                    why = "jumps over a rare block (nested loop or global atomic)" if taken else "exec-mask region, entered"
                else:
                    taken, why = False, "fall-through by default"
                if taken and j == i + 1:
                    taken, why = False, "target is the next block"
                counts["branches taken" if taken else "branches fallen through"] += 1
                notes.append(f"  {label}: {op} .L{target} {'TAKEN' if taken else 'not taken'} ({why})")
                if taken:
                    nxt = j
                    break
            if nxt is None or nxt >= len(blocks):
                notes.append(f"  {label}: the path leaves the kernel's blocks")
                break
            if blocks[nxt][0] == head or (blocks[nxt][0] in seen and nxt != i + 1):
                head_again = blocks[nxt][0]
                done = True
            elif blocks[nxt][0] not in loop:
                notes.append(f"  {label}: the path leaves the loop at {blocks[nxt][0]}")
                break
            i = nxt
        print("  path: " + " ".join(path) + (" -> " + head_again if done else " (open)"))
        print("\n".join(notes))
        order = ("vector", "scalar", "s_nop", "branches taken", "branches fallen through", "wait", "LDS", "vector memory", "scalar memory", "other")
        print("  hot path: " + ", ".join(f"{k} {counts.get(k, 0)}" for k in order) + f"; {sum(counts.values())} instructions")
    got = [(key, re.search(r"; " + key + r": (\d+)", open(args.asm).read().split(name + ":", 1)[1])) for key in ("NumVgprs", "NumSgprs", "ScratchSize", "Occupancy")]
    print("\n" + "  ".join(f"{k} {m.group(1)}" for k, m in got if m))


if __name__ == "__main__":
    main()
