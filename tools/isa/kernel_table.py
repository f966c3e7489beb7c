"""Per-kernel resource table of two builds' device assembly, side by side: the gate of a refactor that must not change what
the compiler makes of a kernel.

    hipcc --offload-arch=gfx950 <the Makefile's FLAGS> --cuda-device-only -S csrc/X.hip -o <dir>/X.s     (old tree and new tree)
    python tools/isa/kernel_table.py <old dir> <new dir> [> profiles/....txt]

Per kernel instantiation: VGPRs (and the waves per SIMD they allow: 512 registers a lane in granules of 8, at most 8 waves), spills,
scratch, LDS, instruction total, MFMA and LDS-DMA instruction counts, and "same text": whether the kernel's instruction stream (body():
labels renumbered, comments dropped) is the old build's.  Exit status 1 if a kernel's text differs, or it moves an occupancy step, spills
or uses scratch MORE THAN BEFORE, changes its LDS size or its MFMA / LDS-DMA counts, or exists on one side only.  Note the spill rule: it is
"no more than the old build", not "none" -- a kernel that spills already (one SGPR in bfp_attention_kernel<32, 1, 2, true> of
mi355q_attention.hip today) passes as long as the new build does not add to it; the columns show both numbers.  (A change that is MEANT
to alter a kernel's code reads the figures and ignores the status; a refactor needs "same text: yes" on every row.)"""
from __future__ import annotations

import re
import subprocess
import sys
from pathlib import Path

META = ("vgpr_count", "agpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size")


def waves(vgprs: int) -> int:
    return max(1, min(8, 512 // max(8, (vgprs + 7) // 8 * 8)))


def demangle(names: list[str]) -> dict[str, str]:
    for tool in ("/opt/rocm/llvm/bin/llvm-cxxfilt", "llvm-cxxfilt", "c++filt"):
        try:
            out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
            return {n: re.sub(r"^void |\(.*$", "", d).replace("mi355q::", "") for n, d in zip(names, out)}
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}


def parse(path: Path) -> dict[str, dict[str, int]]:
    text = path.read_text()
    kernels: dict[str, dict[str, int]] = {}
    # metadata: one YAML map per kernel behind "amdhsa.kernels:", each starting with "  - .agpr_count:" or "  - .args:"
    meta = text[text.rindex("amdhsa.kernels:"):]
    for entry in re.split(r"\n  - ", meta)[1:]:
        if ".symbol:" not in entry:                         # (a list of another section behind the kernels')
            continue
        name = re.search(r"\n    \.name:\s+(\S+)", entry).group(1)
        kernels[name] = {k: int(m.group(1)) if (m := re.search(rf"\.{k}:\s+(\d+)", entry)) else 0 for k in META}
    # bodies: from the kernel's label to its .Lfunc_end
    for name, row in kernels.items():
        start = text.index(f"\n{name}:")
        body = text[start:text.index(".Lfunc_end", start)]
        ins = [ln.split()[0] for ln in body.split("\n") if ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;")]
        row["instructions"] = len(ins)
        row["v_mfma"] = sum(i.startswith("v_mfma") for i in ins)
        row["global_load_lds"] = sum(i.startswith("global_load_lds") for i in ins)
    return kernels


def body(path: Path, name: str) -> list[str]:
    """the kernel's instructions without labels, comments and the symbol names that differ between twins"""
    text = path.read_text()
    start = text.index(f"\n{name}:")
    lines = text[start:text.index(".Lfunc_end", start)].split("\n")
    ins = [ln.split(";")[0].strip() for ln in lines if ln.startswith("\t") and ln.strip()[:1] not in (".", ";")]
    return [re.sub(r"\.LBB\d+_", ".LBB_", i) for i in ins]


def main() -> int:
    old_dir, new_dir = Path(sys.argv[1]), Path(sys.argv[2])
    bad = 0
    cols = ("vgpr_count", "waves", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
            "instructions", "v_mfma", "global_load_lds")
    short = ("vgpr", "waves", "vspill", "sspill", "scratch", "lds", "insts", "mfma", "ldsdma")
    print("old / new per column; waves = waves per SIMD the VGPR count allows")
    for old_s in sorted(old_dir.glob("*.s")):
        new_s = new_dir / old_s.name
        old, new = parse(old_s), parse(new_s)
        names = demangle(sorted(set(old) | set(new)))
        print(f"\n== {old_s.name}: {len(old)} kernels, instructions {sum(r['instructions'] for r in old.values())} -> "
              f"{sum(r['instructions'] for r in new.values())}")
        print("  ".join(f"{s:>11}" for s in short) + "  same text  kernel")
        for n in sorted(names, key=names.get):
            o, w = old.get(n), new.get(n)
            if o is None or w is None:
                print(f"ONE SIDE ONLY  {names[n]}")
                bad += 1
                continue
            o["waves"], w["waves"] = waves(o["vgpr_count"]), waves(w["vgpr_count"])
            # (spills and scratch: none, or -- where the old build has some already -- no more than there)
            same = body(old_s, n) == body(new_s, n)
            fail = (not same or o["waves"] != w["waves"] or any(w[k] > o[k] for k in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"))
                    or any(o[k] != w[k] for k in ("group_segment_fixed_size", "v_mfma", "global_load_lds")))
            bad += fail
            print("  ".join(f"{str(o[c]) + '/' + str(w[c]):>11}" for c in cols) + f"  {'yes' if same else 'no':>9}  {names[n]}"
                  + ("   <-- FAIL" if fail else ""))
    print(f"\n{'FAIL: ' + str(bad) + ' kernels' if bad else 'ok: every kernel the same text, within the conditions'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
