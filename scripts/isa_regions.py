"""Static instruction counts of the fused kinematic kernel's regions between section stamps.

Input: the timing build's device assembly,
    hipcc --cuda-device-only -S -DVC_TIMING -O3 --offload-arch=gfx950 -Iinclude -Ivehicle-control_amd/csrc \
        vehicle-control_amd/csrc/kin_ltv.hip -o kin_ltv_timing.s
The kernel's text is split at each s_memtime (one per VC_TSTAMP / VC_TACC, in program order); each
region is labelled with the source line of the stamp that opens it (from the .loc lines, if the
assembly has them) and counted by instruction class -- the last three columns are the scalar
instructions (s_* other than s_waitcnt / s_nop), the s_nop padding, and the vector instructions no
other class names.  Counts are static: both arms of a uniform
branch inside a region are in it, and a loop body counts once.

With --blocks the input is the PRODUCTION build's assembly (no -DVC_TIMING: the timing build's
register allocation differs) and the kernel's text is split at its basic-block labels instead, one
row per block: its label, the source lines its .loc entries span (if the assembly has them), and
the same classes.  The interior-point loop's blocks are the ones between the lines of its head and
of the second Mehrotra pass's update; a block that a loop executes twice (the pass body) counts once.

usage: python scripts/isa_regions.py kin_ltv_timing.s [min_instr]
       python scripts/isa_regions.py --blocks kin_ltv.s [min_instr]
"""
import re
import sys

CLASSES = [
    ("f64", re.compile(r"^v_\w+_f64")),
    ("v_cndmask", re.compile(r"^v_cndmask")),
    ("agpr mov", re.compile(r"^v_accvgpr_(read|write|mov)")),
    ("lane ops", re.compile(r"^(v_readlane|v_writelane|v_readfirstlane|ds_bpermute|ds_permute|ds_swizzle)|\b(row_shr|row_shl|row_bcast|quad_perm|row_ror|wave_sh)")),
    ("ds_read", re.compile(r"^ds_read")),
    ("ds_write", re.compile(r"^ds_write")),
    ("mfma", re.compile(r"^v_mfma")),
    ("s_waitcnt", re.compile(r"^s_waitcnt")),
    # the scalar unit's own work, its padding, and whatever vector work no class above names: a cut
    # that trades vector instructions for scalar ones (a lane set decided by s_mov instead of
    # v_cmp) shows as such instead of as a smaller "instr" alone
    ("scalar", re.compile(r"^s_(?!waitcnt|nop)")),
    ("s_nop", re.compile(r"^s_nop")),
    ("other vec", None),
]
# "other vec": v_* / ds_* / memory instructions matched by no class above
VECTOR = re.compile(r"^(v_|ds_|global_|flat_|buffer_|scratch_)")


def main():
    argv = [a for a in sys.argv[1:] if a != "--blocks"]
    blocks = len(argv) != len(sys.argv) - 1
    path = argv[0]
    min_instr = int(argv[1]) if len(argv) > 1 else 0
    lines = open(path).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN2vc14kin_ltv_kernel\w*:", l))
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    regions, cur, loc = [], {"open": "entry", "n": 0}, "?"
    for l in lines[start + 1:end]:
        t = l.strip()
        m = re.match(r"\.loc\s+\d+\s+(\d+)", t)
        if m:
            loc = m.group(1)
            if blocks and m.group(1) != "0":
                cur["lo"] = min(cur.get("lo", 1 << 30), int(loc))
                cur["hi"] = max(cur.get("hi", 0), int(loc))
            continue
        m = re.match(r"^(\.LBB\d+_\d+):", t)
        if blocks and m:
            regions.append(cur)
            cur = {"open": m.group(1), "n": 0}
            continue
        if not t or t.startswith((";", ".", "//")) or t.endswith(":"):
            continue
        if not blocks and t.startswith("s_memtime"):
            regions.append(cur)
            cur = {"open": f"line {loc}", "n": 0}
            continue
        cur["n"] += 1
        hit = False
        for name, rx in CLASSES:
            if rx is not None and rx.search(t):
                cur[name] = cur.get(name, 0) + 1
                hit = True
        if not hit and VECTOR.match(t):
            cur["other vec"] = cur.get("other vec", 0) + 1
    regions.append(cur)
    if blocks:
        for r in regions:
            r["open"] += f" (lines {r['lo']}-{r['hi']})" if "lo" in r else ""
    hdr = ["#", "block" if blocks else "opened at", "instr"] + [c for c, _ in CLASSES]
    print("| " + " | ".join(hdr) + " |")
    print("|" + "---|" * len(hdr))
    for i, r in enumerate(regions):
        if r["n"] < min_instr:
            continue
        print("| " + " | ".join([str(i), r["open"], str(r["n"])] + [str(r.get(c, 0)) for c, _ in CLASSES]) + " |")
    print(f"total instructions {sum(r['n'] for r in regions)}, {'blocks' if blocks else 'stamps'} "
          f"{len(regions) - (0 if blocks else 1)}")


if __name__ == "__main__":
    main()
