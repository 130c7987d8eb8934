"""Register / LDS / scratch budget and kernarg preload length of every kernel of libtgis_hip.so, from hipcc's
-Rpass-analysis=kernel-resource-usage remarks and the kernel descriptors of the ISA listing (cross-compiles: needs no GPU).
   python tools/kernel_resources.py > profiles/rNN_kernel_resources.txt
   python tools/kernel_resources.py --csrc OTHER/csrc --no-preload      (another tree, built without the preload flag)"""
import argparse
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "text-generation-inference_amd", "csrc")
# as __graft_entry__.build() and tools/build.sh compile the units of tools/preload_units.txt
PRELOAD = ["-mllvm", "-amdgpu-kernarg-preload-count=16"]
FIELDS = [("Function Name", "name"), ("TotalSGPRs", "sgpr"), ("VGPRs", "vgpr"), ("AGPRs", "agpr"),
          ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=CSRC)
    ap.add_argument("--no-preload", action="store_true", help="compile without the kernarg preload flag")
    ap.add_argument("--only", default=None, help="regular expression: print matching kernels only")
    args = ap.parse_args()
    print("file | kernel | SGPR | VGPR | AGPR | scratch B/lane | waves/SIMD | static LDS B/block | preloaded kernarg dwords")
    with open(os.path.join(ROOT, "tools", "preload_units.txt")) as fh:
        units = [] if args.no_preload else [ln.strip() for ln in fh if ln.strip() and not ln.startswith("#")]
    for src in sorted(glob.glob(os.path.join(args.csrc, "*.hip"))):
        p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC",
                            *(PRELOAD if os.path.basename(src) in units else []),
                            "--cuda-device-only", "-S", src, "-o", "-", "-Rpass-analysis=kernel-resource-usage"],
                           capture_output=True, text=True)
        # kernel descriptors of the listing: .amdhsa_kernel <symbol> ... .amdhsa_user_sgpr_kernarg_preload_length <n>
        preload = {}
        sym = None
        for line in p.stdout.splitlines():
            m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
            if m:
                sym = m.group(1)
            m = re.match(r"\s*\.amdhsa_user_sgpr_kernarg_preload_length\s+(\d+)", line)
            if m and sym:
                preload[sym] = m.group(1)
        cur = {}
        rows = []
        for line in p.stderr.splitlines():
            m = re.search(r"remark: [^:]*:\d+:\d+: +(.*?): (\S+) \[-Rpass-analysis", line) or \
                re.search(r"remark: +(.*?): (\S+) \[-Rpass-analysis", line)
            if not m:
                continue
            for label, key in FIELDS:
                if m.group(1).strip() == label:
                    if key == "name" and cur:
                        rows.append(cur)
                        cur = {}
                    cur[key] = m.group(2)
        if cur:
            rows.append(cur)
        for r in rows:
            name = subprocess.run(["c++filt", r.get("name", "?")], capture_output=True, text=True).stdout.strip()
            name = re.sub(r"\(anonymous namespace\)::", "", name)
            name = re.sub(r"\(.*\)$", "", name)[:110]
            if args.only and not re.search(args.only, name):
                continue
            print(f"{os.path.basename(src)} | {name} | {r.get('sgpr')} | {r.get('vgpr')} | {r.get('agpr')} | {r.get('scratch')} | "
                  f"{r.get('occ')} | {r.get('lds')} | {preload.get(r.get('name'), '?')}")


if __name__ == "__main__":
    main()
