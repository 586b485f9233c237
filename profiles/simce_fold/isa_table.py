"""The device-code table of README.md: per kernel of two gfx950 assembly files (parent, new) one row each.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Wno-unused-value -Iinclude -S --cuda-device-only clip_dplm_amd/csrc/F.hip -o F.s
    python profiles/simce_fold/isa_table.py parent/F.s new/F.s

A kernel's body is everything from its label to its .Lfunc_end (every exit included); kernels are matched by mangled
name.  Columns: instructions, the compiler's NumVgprs / NumAgprs / .amdhsa_next_free_vgpr / TotalNumSgprs, static LDS
bytes, scratch bytes per lane, Occupancy (waves per SIMD), and counts of v_mfma*, global_load*, global_store*,
ds_read*, ds_write*, v_exp* / v_log*.  IDENTICAL: the same instruction stream, symbol names and the function index of
branch labels normalised as tools/compare_kernel_isa.py does.  Under a kernel with scratch: every scratch_ instruction
with the basic block it lies in and that block's loop annotation (none: outside every loop).
"""
import re
import subprocess
import sys

COLS = ["instr", "vgpr", "agpr", "next_free", "sgpr", "lds", "scratch", "waves", "mfma", "gld", "gst", "dsr", "dsw", "explog"]


def demangle(name):
    try:
        s = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        return s.replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0] or name
    except OSError:
        return name


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)^; Occupancy: (\d+)", txt, flags=re.S | re.M):
        name, body, meta, occ = m.groups()
        desc = re.search(r"\.amdhsa_kernel " + re.escape(name) + r"\n(.*?)\.end_amdhsa_kernel", txt, flags=re.S)
        if not desc:
            continue
        lines = [l.strip() for l in body.splitlines() if l.strip()]
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", l)) for l in lines if not l.startswith((";", "."))]
        num = lambda pat, s: int(re.search(pat + r":? +(\d+)", s).group(1))
        count = lambda pat: sum(1 for i in ins if re.match(pat, i))
        d = dict(instr=len(ins), vgpr=num("; NumVgprs", meta), agpr=num("; NumAgprs", meta),
                 next_free=num(r"\.amdhsa_next_free_vgpr", desc.group(1)), sgpr=num("; TotalNumSgprs", meta),
                 lds=num(r"\.amdhsa_group_segment_fixed_size", desc.group(1)),
                 scratch=num(r"\.amdhsa_private_segment_fixed_size", desc.group(1)), waves=int(occ),
                 mfma=count("v_mfma"), gld=count("global_load"), gst=count("global_store"), dsr=count("ds_read"),
                 dsw=count("ds_write"), explog=count("v_exp|v_log"))
        block, in_loop, spills, first, last = "entry", False, [], None, None
        for n, l in enumerate(lines):
            b = re.match(r"(\.LBB\d+_\d+:|; %bb\.\d+:)(.*)", l)
            if b:
                block = (b.group(1) + " " + " ".join(b.group(2).replace(";", " ").split())).strip()
                in_loop = "Loop" in l
                if in_loop and first is None:
                    first = n
            elif l.startswith("scratch_"):
                spills.append(f"line {n}: {l.split(';')[0].strip()}   [block {block}]")
            if in_loop:
                last = n
        if spills:
            spills.append(f"blocks annotated as in a loop: lines {first} to {last} of {len(lines)}")
        d["spills"], d["ins"] = spills, ins
        out[name] = d
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    for name, d in new.items():
        row = lambda tag, k, verdict: print(f"| {demangle(name)} | {tag} | " + " | ".join(str(k[c]) for c in COLS) + f" | {verdict} |")
        if name in old:
            row("parent", old[name], "")
            row("new", d, "IDENTICAL" if old[name]["ins"] == d["ins"] else "differs")
            for tag, k in (("parent", old[name]), ("new", d)):
                for s in k["spills"]:
                    print(f"    {tag}: {s}")
        else:
            row("new only", d, "NEW KERNEL")
    for name in old:
        if name not in new:
            print(f"| {demangle(name)} | parent only | " + " | ".join(str(old[name][c]) for c in COLS) + " | GONE |")


if __name__ == "__main__":
    main()
