"""Compare two compiler resource reports of the device code (`make -C snail_amd/csrc asm` writes snail_amd/csrc/snail_hip.resources): per
kernel of the project's own namespaces (dev, dev_sse, dev_heat, ...; library kernels such as rocprim's are left out) VGPRs, SGPRs, scratch
bytes per lane, VGPR spills, SGPR spills and occupancy -- before | after -- for every kernel the BEFORE report has, then the kernels only
the AFTER report has.  Exit status 1 if a kernel of the before report is missing or differs.

    make -C snail_amd/csrc asm && cp snail_amd/csrc/snail_hip.resources before.resources      # on the commit to compare against
    make -C snail_amd/csrc asm                                                                # on this one
    python tools/resource_diff.py before.resources snail_amd/csrc/snail_hip.resources > profiles/materials_resources.txt"""
import re
import subprocess
import sys

FIELDS = ("VGPRs", "TotalSGPRs", "ScratchSize [bytes/lane]", "VGPRs Spill", "SGPRs Spill", "Occupancy [waves/SIMD]")


def parse(path):
    out, cur = {}, None
    for line in open(path):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            out[cur] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\S+) \[-Rpass", line)
        if m and cur:
            out[cur][m.group(1).strip()] = m.group(2)
    return out


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    names = sorted(set(before) | set(after))
    plain = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    own = [(n, d) for n, d in zip(names, plain) if "rocprim" not in d and "hipcub" not in d]
    row = lambda r: " ".join("%4s" % r.get(k, "?") for k in FIELDS)      # noqa: E731
    old = [(n, d) for n, d in own if n in before]
    bad = [d for n, d in old if before[n] != after.get(n)]
    print("Compiler's resource report of the project's kernels: VGPRs, SGPRs, scratch bytes/lane, VGPR spills, SGPR spills, occupancy -- before | after.")
    print("%d kernels in the before report, %d of them missing or different after; %d new kernels." % (len(old), len(bad), len(own) - len(old)))
    print()
    for n, d in sorted(old, key=lambda x: x[1]):
        print("%s | %s  %s%s" % (row(before[n]), row(after.get(n, {})), re.sub(r"^void ", "", d), "" if before[n] == after.get(n) else "   <-- DIFFERS"))
    print()
    print("new:")
    for n, d in sorted(own, key=lambda x: x[1]):
        if n not in before:
            print("%s | %s  %s" % (" " * len(row({})), row(after[n]), re.sub(r"^void ", "", d)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
