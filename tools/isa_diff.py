#!/usr/bin/env python
"""Are the kernels of two gfx950 assembly files (hipcc <build.py's flags> --offload-device-only -S) the same kernels?
    python tools/isa_diff.py parent.s branch.s
Per kernel symbol: the same symbols on both sides; VGPRs, AGPRs, scratch, spills, LDS and occupancy identical; the histogram of
every v_* (MFMA included), ds_*, global_* / buffer_* / flat_* / scratch_* opcode identical -- a refactor of device code that keeps
these moved no vector instruction and no register.  Scalar instructions, SGPRs, s_waitcnt and s_nop may differ and are reported.
Exit status 1 when a kernel fails (function splitting and opcode classes: tools/isa_mix.py)."""
import re, sys
from collections import Counter

STRICT = ("NumVgprs", "NumAgprs", "ScratchSize", "Occupancy", "LDSByteSize", "VGPRSpill", "SGPRSpill")   # "; <key>: <n>" lines
LOOSE = ("TotalNumSgprs",)
VECTOR = ("v_", "ds_", "global_", "buffer_", "flat_", "scratch_")


def kernels(path):
    txt = open(path).read()
    spills = {}   # the code object's metadata: one "- .agpr_count: ..." entry per kernel
    for e in re.split(r"^  - \.agpr_count:", txt, flags=re.M)[1:]:
        name = re.search(r"\.name:\s+(\w+)", e).group(1)
        spills[name] = {k: int(re.search(r"\." + f + r":\s+(\d+)", e).group(1)) for k, f in (("VGPRSpill", "vgpr_spill_count"), ("SGPRSpill", "sgpr_spill_count"))}
    starts = list(re.finditer(r"^(\w+):\s*;\s*@\1\n", txt, re.M))
    out = {}
    for i, m in enumerate(starts):
        name = m.group(1)
        seg = txt[m.end():starts[i + 1].start() if i + 1 < len(starts) else len(txt)]
        body, _, tail = seg.partition(".Lfunc_end")
        if "; Kernel info:" not in tail:
            continue
        ops = Counter()
        for l in body.splitlines():
            t = l.strip()
            if t and not t.startswith((";", ".")) and not t.endswith(":"):
                ops[t.split()[0]] += 1
        res = dict(spills[name])
        for k in STRICT[:5] + LOOSE:
            res[k] = int(re.search(r";\s*" + k + r":\s*(\d+)", tail).group(1))
        out[name] = (ops, res)
    return out


def main(pa, pb):
    A, B = kernels(pa), kernels(pb)
    bad = 0
    for n in sorted(set(A) ^ set(B)):
        print(f"FAIL {n}: only in {'parent' if n in A else 'branch'}")
        bad += 1
    loose = Counter()
    for n in sorted(set(A) & set(B)):
        (oa, ra), (ob, rb) = A[n], B[n]
        why = [f"{k} {ra[k]} -> {rb[k]}" for k in STRICT if ra[k] != rb[k]]
        why += [f"{op} {oa[op]} -> {ob[op]}" for op in sorted(set(oa) | set(ob)) if op.startswith(VECTOR) and oa[op] != ob[op]]
        if why:
            print(f"FAIL {n}: " + "; ".join(why))
            bad += 1
        if ra["TotalNumSgprs"] != rb["TotalNumSgprs"]:
            loose["kernels whose SGPR count changed"] += 1
        for op in set(oa) | set(ob):
            if not op.startswith(VECTOR) and oa[op] != ob[op]:
                loose[op] += ob[op] - oa[op]
    note = ", ".join(f"{k} {v:+d}" if k.startswith("s_") else f"{k}: {v}" for k, v in sorted(loose.items())) or "no scalar difference"
    print(f"{'FAIL' if bad else 'same'}: {len(set(A) & set(B))} kernels, {bad} failed; allowed differences: {note}")
    return 1 if bad or not A else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
