"""Compare the gfx950 instruction streams of the kernels in two device-assembly files, kernel by kernel.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -S --cuda-device-only clip_dplm_amd/csrc/simce_tiled.hip -o new.s
    (the same in a checkout of the other commit -> old.s)
    python tools/compare_kernel_isa.py old.s new.s

A kernel is matched by its mangled name with trailing `false` template arguments (`Lb0E`) added by the newer file
ignored; labels, directives and comments are dropped, symbol names and the function index of branch labels inside
instructions are normalised.  Prints per
kernel the instruction counts and IDENTICAL / differs / new, and each kernel's scratch size.  Exit status 1 if a kernel
present in both files differs.
"""
import re
import sys


def kernels(path):
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):.*?\n(.*?)s_endpgm", txt, flags=re.S | re.M):
        ins = [re.sub(r"\.LBB\d+_", ".LBB_", re.sub(r"_Z\w+", "SYM", l.strip())) for l in m.group(2).splitlines()
               if l.strip() and not l.strip().startswith((";", "."))]
        scratch = re.search(r"\.amdhsa_kernel " + re.escape(m.group(1)) + r"\n.*?private_segment_fixed_size (\d+)", txt, flags=re.S)
        out[m.group(1)] = (ins, int(scratch.group(1)) if scratch else -1)
    return out


def key(name):
    """The mangled name with trailing `false` boolean template arguments dropped (none left: the non-template name)."""
    def f(m):
        args = re.sub(r"(Lb0E)+$", "", m.group(1))
        return "I" + args + "EEv" if args else "E"
    return re.sub(r"I((?:Lb[01]E)+)EEv", f, name, count=1)


def main():
    old = {key(k): v for k, v in kernels(sys.argv[1]).items()}
    new = kernels(sys.argv[2])
    bad = 0
    for name, (ins, scratch) in new.items():
        match = key(name) if key(name) in old else None
        if match is None:
            print(f"{name[:78]:78s} {len(ins):6d}      - new        scratch {scratch} B")
            continue
        same = old[match][0] == ins
        bad += not same
        print(f"{name[:78]:78s} {len(ins):6d} {len(old[match][0]):6d} {'IDENTICAL' if same else 'differs  '}  scratch {scratch} B")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
