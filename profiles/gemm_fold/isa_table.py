"""The device-code table of README.md: per kernel of two gfx950 assembly files (parent, new) one row each.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value -Iinclude -S --cuda-device-only clip_dplm_amd/csrc/F.hip -o F.s
    python profiles/gemm_fold/isa_table.py parent/F.s new/F.s [--diff]

A kernel's body is everything from its label to its .Lfunc_end (every exit included); kernels are matched by mangled
name.  Columns, the ones the adoption rule of the fold names: instructions, NumVgprs, NumAgprs, scratch bytes per lane,
the metadata's .vgpr_spill_count, static LDS bytes (the GEMM kernels' LDS is dynamic: 0), Occupancy (waves per SIMD), and
counts of v_mfma*, buffer_load*lds, global_load*lds, buffer_store*, global_store*, ds_read*, ds_write*, s_barrier,
s_waitcnt, s_setprio.  Verdict: IDENTICAL (the same instruction stream, symbol names and the function index of branch
labels normalised as tools/compare_kernel_isa.py does), "scalar only" (every vector, LDS, memory, branch, barrier, wait and
priority instruction is where it was, in the same order with the same vector registers and immediates - the streams are
equal once the scalar instructions other than s_barrier / s_waitcnt / s_setprio / s_sleep are taken out and SGPR
operands are spelt alike - and no scalar instruction that a line diff adds or removes lies in a block the compiler
annotates as inside a loop at depth > 1, the K loop of the persistent kernels: depth 1 is their tile loop), or "differs".
--diff prints the unified diff of every kernel that is not IDENTICAL.  Under a kernel with scratch: every scratch_
instruction with the basic block it lies in.
"""
import difflib
import re
import subprocess
import sys

COLS = ["instr", "vgpr", "agpr", "scratch", "spills", "lds", "waves", "mfma", "bld_lds", "gld_lds", "bst", "gst", "dsr",
        "dsw", "barrier", "waitcnt", "setprio"]
KEEP = ("s_barrier", "s_waitcnt", "s_setprio", "s_sleep")


def demangle(name):
    try:
        s = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        return s.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] or name
    except OSError:
        return name


def kernels(path):
    txt = open(path).read()
    out = {}
    spilled = {m.group(1): int(m.group(2)) for m in                    # the code object's metadata, per kernel
               re.finditer(r"\.name: +(\w+)\n(?:(?!\.name:).*\n)*? +\.vgpr_spill_count: +(\d+)", txt)}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)^; Occupancy: (\d+)", txt, flags=re.S | re.M):
        name, body, meta, occ = m.groups()
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, flags=re.S)
        if not desc:
            continue
        lines = [l.strip() for l in body.splitlines() if l.strip()]
        norm = lambda l: re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", l))
        ins, depth_of, scratch_lines, block, depth = [], [], [], "entry", 0
        for l in lines:
            b = re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)(.*)", l)
            if b:
                block = b.group(1)
                d = re.search(r"Depth[= ](\d+)", l)
                depth = int(d.group(1)) if d else 0
                continue
            h = re.search(r"This (?:Inner )?Loop Header: Depth=(\d+)", l)      # an inner loop's header: on the line after its label
            if h and l.startswith(";"):
                depth = int(h.group(1))
            if l.startswith((";", ".")):
                continue
            ins.append(norm(l.split(";")[0].strip()))
            depth_of.append(depth)
            if l.startswith("scratch_"):
                scratch_lines.append(f"instruction {len(ins)}: {l.split(';')[0].strip()}   [block {block}, loop depth {depth}]")
        num = lambda pat, s: int(re.search(pat + r":? +(\d+)", s).group(1))
        count = lambda pat: sum(1 for i in ins if re.match(pat, i))
        d = dict(instr=len(ins), vgpr=num("; NumVgprs", meta), agpr=num("; NumAgprs", meta),
                 scratch=num(r"\.amdhsa_private_segment_fixed_size", desc.group(1)), spills=spilled.get(name, -1),
                 lds=num(r"\.amdhsa_group_segment_fixed_size", desc.group(1)), waves=int(occ),
                 mfma=count("v_mfma"), bld_lds=count(r"buffer_load.* lds"), gld_lds=count(r"global_load_lds"),
                 bst=count("buffer_store"), gst=count("global_store"), dsr=count("ds_read"), dsw=count("ds_write"),
                 barrier=count("s_barrier"), waitcnt=count("s_waitcnt"), setprio=count("s_setprio"))
        d.update(ins=ins, depth_of=depth_of, scratch_lines=scratch_lines, maxdepth=max(depth_of, default=0))
        out[name] = d
    return out


def is_scalar_alu(i):
    return i.startswith("s_") and not i.startswith(KEEP)


def skeleton(k):
    """The stream without its scalar ALU / move / load instructions and with every SGPR operand of what remains spelt S."""
    return [re.sub(r"\bs\[\d+:\d+\]|\bs\d+\b", "S", i) for i in k["ins"] if not is_scalar_alu(i)]


def verdict(o, n):
    if o["ins"] == n["ins"]:
        return "IDENTICAL"
    if skeleton(o) != skeleton(n):
        return "differs"
    sm = difflib.SequenceMatcher(a=o["ins"], b=n["ins"], autojunk=False)
    for tag, i1, i2, j1, j2 in sm.get_opcodes():
        if tag == "equal":
            continue
        for k, seq, lo, hi in ((o, o["ins"], i1, i2), (n, n["ins"], j1, j2)):
            if any(is_scalar_alu(seq[x]) and k["depth_of"][x] > 1 for x in range(lo, hi)):
                return "differs"
    return "scalar only"


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    for name, d in new.items():
        row = lambda tag, k, v: print(f"| {demangle(name)} | {tag} | " + " | ".join(str(k[c]) for c in COLS) + f" | {v} |")
        if name not in old:
            row("new only", d, "NEW KERNEL")
            continue
        v = verdict(old[name], d)
        row("parent", old[name], "")
        row("new", d, v)
        for tag, k in (("parent", old[name]), ("new", d)):
            for s in k["scratch_lines"]:
                print(f"    {tag}: {s}")
        if v != "IDENTICAL" and "--diff" in sys.argv:
            print("\n".join(difflib.unified_diff(old[name]["ins"], d["ins"], "parent", "new", n=1, lineterm="")))
    for name in old:
        if name not in new:
            print(f"| {demangle(name)} | parent only | " + " | ".join(str(old[name][c]) for c in COLS) + " | GONE |")


if __name__ == "__main__":
    main()
