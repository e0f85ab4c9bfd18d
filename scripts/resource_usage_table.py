"""Kernel resource usage from hipcc's -Rpass-analysis=kernel-resource-usage remarks, one line per kernel instantiation.

    cd psi-gnn_amd/csrc; R=EXTRA=-Rpass-analysis=kernel-resource-usage
    make clean; make ../libpsignn_hip.so $R 2> d10.log; make ../libpsignn_hip_d8.so $R 2> d8.log; make ../libpsignn_hip_d16.so $R 2> d16.log
    python scripts/resource_usage_table.py d10.log                                # table of one build
    python scripts/resource_usage_table.py before.log d10.log 8:d8.log 16:d16.log  # width 10 before / after, then the other widths

Needs no GPU.  One log per library (the remarks of one compile carry no width); kernels are keyed by translation unit and
mangled name.
"""
import re
import sys

FIELDS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]"]
SHORT = ["SGPR", "VGPR", "AGPR", "scratch", "occ", "sspill", "vspill", "LDS"]


def parse(path, width=10):
    out, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.match(r"(\S+?):\d+:\d+: remark: Function Name: (\S+)", line)
        if m:
            cur = (m.group(1), width, m.group(2))
            out[cur] = {}
            continue
        m = re.match(r"\S+: remark:\s+(.+?): (\S+) \[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            out[cur][m.group(1)] = m.group(2)
    return out


def demangle(names):
    import shutil
    import subprocess
    filt = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        r = subprocess.run([filt], input="\n".join(names), capture_output=True, text=True, check=True)
        return [re.sub(r"\(.*", "", s) for s in r.stdout.splitlines()]
    except Exception:
        return list(names)


def table(res, only=None):
    keys = sorted(k for k in res if only is None or only(k))
    names = demangle([k[2] for k in keys])
    rows = [f"{'file':18s} {'d':>2s} " + " ".join(f"{s:>7s}" for s in SHORT) + "  kernel"]
    for k, n in zip(keys, names):
        rows.append(f"{k[0]:18s} {k[1]:2d} " + " ".join(f"{res[k].get(f, '?'):>7s}" for f in FIELDS) + "  " + n)
    return "\n".join(rows)


if __name__ == "__main__":
    if len(sys.argv) == 2:
        print(table(parse(sys.argv[1])))
    else:
        a, b = parse(sys.argv[1]), parse(sys.argv[2])
        diff = [k for k in sorted(set(a) | set(b)) if a.get(k) != b.get(k)]
        print(f"width-10 kernel instantiations: {len(a)} before, {len(b)} after; differing or missing: {len(diff)}")
        for k in diff:
            print("  DIFF", k[0], k[2], "before", a.get(k), "after", b.get(k))
        print("\n== width 10, after (identical to before unless listed above) ==")
        print(table(b))
        for arg in sys.argv[3:]:
            w, path = arg.split(":", 1)
            print(f"\n== width {w} ==")
            print(table(parse(path, int(w))))
