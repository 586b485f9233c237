"""The speed table of README.md from the outputs of `tools/bench_kernels.py gemm`, three runs of each tree:

    python profiles/gemm_fold/speed_table.py parent_1.log parent_2.log parent_3.log -- new_1.log new_2.log new_3.log

One row per (shape, epilogue, arm): the parent's runs, their min-max and median, the new tree's runs and median, and whether
the new median lies inside the parent's own min-max or below it (the margin is the parent's spread and nothing else).
"""
import re
import statistics
import sys


def rows(path):
    out, arms = {}, []
    for line in open(path):
        cells = [c.strip() for c in line.rstrip("\n").split("|")]
        if line.startswith("shape"):
            arms = [c.split()[0] for c in cells[1:-1]]
            continue
        m = re.match(r"(.{12}) +(\d+) +(\d+) +(\d+) +(\S+)$", cells[0])
        if not m or len(cells) < 2:
            continue
        key = (m.group(1).strip(), f"{m.group(3)}x{m.group(4)}", m.group(5))
        if cells[1].startswith("generic-K"):
            out[key + ("generic-K",)] = float(cells[1].split()[1])
        else:
            for arm, c in zip(arms, cells[1:]):
                out[key + (arm,)] = float(c.split()[0])
    return out


def main():
    cut = sys.argv.index("--")
    old, new = [rows(p) for p in sys.argv[1:cut]], [rows(p) for p in sys.argv[cut + 1:]]
    print("| shape | N x K | epilogue | arm | parent runs (us) | parent min-max | parent median | new runs (us) | new median | new - parent | inside or below |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    outside = 0
    for key in old[0]:
        o, n = [r[key] for r in old], [r[key] for r in new]
        om, nm = statistics.median(o), statistics.median(n)
        ok = nm <= max(o)
        outside += not ok
        print(f"| {key[0]} | {key[1]} | {key[2]} | {key[3]} | " + " / ".join(f"{v:.1f}" for v in o) + f" | {min(o):.1f} - {max(o):.1f} | {om:.1f} | "
              + " / ".join(f"{v:.1f}" for v in n) + f" | {nm:.1f} | {nm - om:+.1f} | {'yes' if ok else 'NO'} |")
    print(f"rows whose new median lies above the parent's max: {outside}")


if __name__ == "__main__":
    main()
