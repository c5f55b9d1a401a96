"""Resource table of the kernels of the given csrc/*.hip files: compiles each for the device only with
the build's flags plus -Rpass-analysis=kernel-resource-usage and prints one row per kernel (VGPRs,
AGPRs, spills, scratch, occupancy, LDS). No GPU needed.

usage: python tools/kernel_resources.py [--csrc DIR] corr.hip uvfused.hip > profiles/corr_shared/resources_after.txt
       python tools/kernel_resources.py winoconv3.hip winoconv.hip convfew.hip
--csrc DIR: read the sources from DIR (an archive of another commit) instead of the tree's csrc."""
import re
import subprocess
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
from transplat_amd import build  # noqa: E402

FIELDS = ["VGPRs", "AGPRs", "VGPRs Spill", "SGPRs Spill", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
          "LDS Size [bytes/block]"]
args = sys.argv[1:]
csrc = build.CSRC
if args[:1] == ["--csrc"]:
    csrc, args = Path(args[1]), args[2:]
if not args:
    sys.exit(__doc__)
print("| Kernel | VGPRs | AGPRs | VGPR spill | SGPR spill | Scratch | Occupancy | LDS (bytes) |")
print("|---|---|---|---|---|---|---|---|")
for name in args:
    cmd = [build._hipcc(), *build.HIPCC_FLAGS, f"-I{csrc}", *build.FILE_FLAGS.get(name, []), "--cuda-device-only",
           "-Rpass-analysis=kernel-resource-usage", "-c", str(csrc / name), "-o", "/dev/null"]
    done = subprocess.run(cmd, capture_output=True, text=True)
    if done.returncode:
        sys.exit("\n".join(line for line in done.stderr.splitlines() if "remark:" not in line))
    err = done.stderr
    rows, cur = [], None
    for line in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            cur = {"name": m.group(1)}
            rows.append(cur)
        m = re.search(r"remark:\s+([A-Za-z \[\]/]+): (\d+)", line)
        if m and cur is not None:
            cur[m.group(1).strip()] = m.group(2)
    names = subprocess.run(["c++filt"], input="\n".join(r["name"] for r in rows), capture_output=True,
                           text=True).stdout.split("\n")
    for r, full in zip(rows, names):
        short = re.sub(r"^void |tsplat::|\(.*\)$", "", full)
        print(f"| `{short}` | " + " | ".join(r.get(f, "?") for f in FIELDS) + " |")
