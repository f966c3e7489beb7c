"""kernel_table.py for a change that ADDS a template parameter: the old build's kernels against their twins in the new build -- the
instantiations whose new parameter has the value that must leave the device code alone -- and the new build's other instantiations
against those twins.

    python tools/isa/kernel_twins.py <old dir> <new dir> <suffix> [--rename <regex> <replacement>]... [> profiles/....txt]

<suffix> is what the twin's demangled template argument list ends with behind the old one's, e.g. ", false" (decode_scores_kernel<1,
true> -> decode_scores_kernel<1, true, false>; a kernel that was no template, f -> f<false>).  --rename pairs an old kernel with a
RENAMED one: every pair is applied (re.sub) to the old kernel's demangled name in front of the suffix rule ("" for none), and an old
file that has no file of its name in the new build is held against the kernels of all the new build's files.  Per pair: the figures of kernel_table.py
plus the SGPR count and whether the instruction streams are the same text.  A file only the new build has (with every old file paired
by name) is listed whole, as new instantiations.  Exit status 1 if a twin is missing or differs in VGPRs, SGPRs, spills, scratch, LDS,
MFMA or LDS-DMA counts, or a kernel of a new file spills or uses scratch."""
from __future__ import annotations

import re
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent))
from kernel_table import body, demangle, parse, waves  # noqa: E402

COLS = ("vgpr_count", "sgpr_count", "waves", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size",
        "group_segment_fixed_size", "instructions", "v_mfma", "global_load_lds")
SHORT = ("vgpr", "sgpr", "waves", "vspill", "sspill", "scratch", "lds", "insts", "mfma", "ldsdma")
MUST = ("vgpr_count", "sgpr_count", "vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size",
        "v_mfma", "global_load_lds")


def twin_of(old_name: str, suffix: str) -> str:
    return old_name[:-1] + suffix + ">" if old_name.endswith(">") else old_name + "<" + suffix.lstrip(", ") + ">"


def main() -> int:
    old_dir, new_dir, suffix = Path(sys.argv[1]), Path(sys.argv[2]), sys.argv[3]
    renames = [(sys.argv[i + 1], sys.argv[i + 2]) for i, a in enumerate(sys.argv) if a == "--rename"]
    bad = 0
    for old_s in sorted(old_dir.glob("*.s")):
        new_files = [new_dir / old_s.name] if (new_dir / old_s.name).exists() else sorted(new_dir.glob("*.s"))
        old, new, where = parse(old_s), {}, {}
        for f in new_files:
            rows = parse(f)
            new.update(rows)
            where.update(dict.fromkeys(rows, f))
        on, nn = demangle(sorted(old)), demangle(sorted(new))
        by_name = {d: m for m, d in nn.items()}
        for rows in (old, new):
            for r in rows.values():
                r["waves"] = waves(r["vgpr_count"])
        print(f"\n== {old_s.name}: {len(old)} kernels before, {len(new)} now; old / twin per column")
        print("  ".join(f"{s:>9}" for s in SHORT) + "  same text  kernel")
        twins = set()
        for m in sorted(old, key=on.get):
            name = on[m]
            for pattern, repl in renames:
                name = re.sub(pattern, repl, name)
            t = (by_name.get(twin_of(name, suffix)) if suffix else None) or by_name.get(name)      # (a kernel the change did not touch keeps its name)
            if t is None:
                print(f"NO TWIN  {on[m]}")
                bad += 1
                continue
            twins.add(t)
            o, w = old[m], new[t]
            fail = any(o[k] != w[k] for k in MUST)
            bad += fail
            same = body(old_s, m) == body(where[t], t)
            print("  ".join(f"{str(o[c]) + '/' + str(w[c]):>9}" for c in COLS) + f"  {'yes' if same else 'no':>9}  {nn[t]}" + ("   <-- FAIL" if fail else ""))
        print("-- new instantiations")
        print("  ".join(f"{s:>9}" for s in SHORT) + "  kernel")
        for m in sorted(set(new) - twins, key=nn.get):
            print("  ".join(f"{new[m][c]:>9}" for c in COLS) + f"  {nn[m]}")
    # files the change ADDS (no old file of the name, and no old file left to be held against them): every kernel is a new instantiation
    if all((new_dir / f.name).exists() for f in old_dir.glob("*.s")):
        for new_s in sorted(f for f in new_dir.glob("*.s") if not (old_dir / f.name).exists()):
            rows = parse(new_s)
            names = demangle(sorted(rows))
            print(f"\n== {new_s.name}: a new file, {len(rows)} kernels")
            print("  ".join(f"{s:>9}" for s in SHORT) + "  kernel")
            for m in sorted(rows, key=names.get):
                rows[m]["waves"] = waves(rows[m]["vgpr_count"])
                extra = rows[m]["vgpr_spill_count"] or rows[m]["sgpr_spill_count"] or rows[m]["private_segment_fixed_size"]
                bad += bool(extra)
                print("  ".join(f"{rows[m][c]:>9}" for c in COLS) + f"  {names[m]}" + ("   <-- FAIL: spills or scratch" if extra else ""))
    print(f"\n{'FAIL: ' + str(bad) + ' kernels' if bad else 'ok: every twin keeps the old figures'}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
