"""Instructions one block of a chain kernel's loop executes, per phase and class, from the
device assembly (CPU only: no GPU is needed).

    python benchmarks/hot_path_counts.py openseize_amd/csrc/chain_zpn_body.h profiles/zpn_epilogue_path_after.txt [-v]
    python benchmarks/hot_path_counts.py kernel.s profiles/zpn_epilogue_path_after.txt [-v]

The first form compiles ONE instance of the kernel to gfx950 assembly with the library's flags
(hipcc -O3 -std=c++17 -fPIC --offload-arch=gfx950 --cuda-device-only -S; about five seconds): the
body up to its dispatchers plus an explicit instantiation of chain_zpn_kernel<27, 6, 2, 5, true>,
the headline's instance (another one: --instance "24, 6, 2, 8, true"; another revision of the body:
git show REV:openseize_amd/csrc/chain_zpn_body.h > /tmp/body.h).  The second form reads such an
assembly file.

The walk starts at the head of the kernel's outermost loop that holds a barrier (the block loop)
and follows the control flow until it is back there.  An unconditional branch is followed; at a
conditional one the walk takes the next line of the path file:

    T [phase]      the branch is taken
    N [phase]      it falls through
    # ...          comment

and, where a phase name follows, counts everything from there on under that phase.  The path file
is the record of WHICH block is counted (steady state: not the run's first block, own, not edge,
not bad, the planner's nh, Rf and R of the benchmark's pair); with -v the walk prints every branch
with the scalar instructions in front of it, which is how the file is written and checked.  When
the file runs out the walk stops and shows where.

Classes, by the mnemonic's prefix alone:  v_*_f64 -> float64 arithmetic;  other v_ -> other
vector;  ds_ -> LDS;  buffer_ / global_ / flat_ / scratch_ -> vector memory;  s_ -> scalar.
"""
import os
import re
import subprocess
import sys
import tempfile

CLASSES = ["f64", "vector", "lds", "vmem", "scalar"]


def classify(op):
    if op.startswith("v_"):
        return "f64" if "_f64" in op else "vector"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "vmem"
    if op.startswith("s_"):
        return "scalar"
    return None


def parse(path):
    """-> list of (lineno, label or None, mnemonic or None, operands, text)"""
    out = []
    for no, line in enumerate(open(path), 1):
        text = line.rstrip("\n")
        code = text.split(";")[0].strip()
        m = re.match(r"^(\.LBB\d+_\d+):", code)
        if m:
            out.append((no, m.group(1), None, "", text))
            continue
        if not code or code.startswith(".") or code.endswith(":"):
            continue
        parts = code.split(None, 1)
        out.append((no, None, parts[0], parts[1] if len(parts) > 1 else "", text))
    return out


def compile_instance(body, inst):
    """The assembly of chain_zpn_kernel<inst> alone, from the kernel body `body`."""
    csrc = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "openseize_amd", "csrc")
    text = open(body).read()
    cut = text.index("// (one translation unit per mode count")
    tmp = tempfile.mkdtemp()
    with open(os.path.join(tmp, "one.hip"), "w") as fh:
        fh.write("#define OSZ_ZPN_NM %s\n" % inst.split(",")[1].strip())
        fh.write(text[:cut])
        fh.write("template __global__ void chain_zpn_kernel<%s>(ZpArgs);\n}  // namespace osz\n" % inst)
    out = os.path.join(tmp, "one.s")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-I", csrc,
                           "-I", os.path.join(csrc, "..", "..", "include"), "--cuda-device-only", "-S",
                           os.path.join(tmp, "one.hip"), "-o", out], stderr=subprocess.DEVNULL)
    return out


def main():
    verbose = "-v" in sys.argv
    args = [a for a in sys.argv[1:] if a != "-v"]
    inst = "27, 6, 2, 5, true"
    if "--instance" in args:
        k = args.index("--instance")
        inst = args[k + 1]
        del args[k:k + 2]
    ins = parse(compile_instance(args[0], inst) if args[0].endswith(".h") else args[0])
    steps = []
    for line in open(args[1]):
        line = line.split("#")[0].split()
        if line:
            steps.append((line[0], line[1] if len(line) > 1 else None))
    label_at = {lab: i for i, (_, lab, _, _, _) in enumerate(ins) if lab}
    # the block loop: the outermost loop with the most basic blocks (the compiler names every
    # block's loop header in a comment)
    size = {}
    for (_, lab, _, _, text) in ins:
        m = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1", text)
        if lab and m:
            size[m.group(1)] = size.get(m.group(1), 0) + 1
    assert size, "no loop found"
    head = label_at[".L" + max(size, key=size.get)]
    counts, order = {}, []
    phase = "transform"
    i, k, seen_head = head, 0, False
    recent = []
    while True:
        no, lab, op, opnd, text = ins[i]
        if i == head and seen_head:
            break
        seen_head = True
        if op is None:
            i += 1
            continue
        cls = classify(op)
        if cls:
            if phase not in counts:
                counts[phase] = dict.fromkeys(CLASSES, 0)
                order.append(phase)
            counts[phase][cls] += 1
        if cls == "scalar":
            recent = (recent + [text.strip()])[-6:]
        if op == "s_branch":
            i = label_at[opnd]
            continue
        if op.startswith("s_cbranch"):
            if k >= len(steps):
                print(f"path file ends at line {no}: {text.strip()}")
                for r in recent:
                    print("      ", r)
                break
            way, ph = steps[k]
            k += 1
            if verbose:
                print(f"[{k}] line {no} {op} {opnd} -> {way} {ph or ''}")
                for r in recent[:-1]:
                    print("      ", r)
            if ph:
                phase = ph
            i = label_at[opnd] if way == "T" else i + 1
            continue
        if op in ("s_endpgm", "s_setpc_b64"):
            print(f"left the loop at line {no}")
            break
        i += 1
    print(f"{'phase':28s}" + "".join(f"{c:>9s}" for c in CLASSES) + f"{'v_ all':>9s}")
    tot = dict.fromkeys(CLASSES, 0)
    for ph in order:
        c = counts[ph]
        print(f"{ph:28s}" + "".join(f"{c[x]:9d}" for x in CLASSES) + f"{c['f64'] + c['vector']:9d}")
        for x in CLASSES:
            tot[x] += c[x]
    print(f"{'one block':28s}" + "".join(f"{tot[x]:9d}" for x in CLASSES) + f"{tot['f64'] + tot['vector']:9d}")


if __name__ == "__main__":
    main()
