#!/usr/bin/env python3
"""tools/lab/aux_sites.py <parent.s> <arm.s> ... — where a cache-policy macro of k_flatten.hip lands in the gfx950 assembly (no GPU needed).

Input: device assembly of k_flatten.hip (hipcc ... --cuda-device-only -S, the Makefile's flags plus the arm's -D).  Per kernel the script counts the buffer
instructions by opcode and by policy bits (nt / sc0 / sc1) and prints every kernel whose counts differ from the first file's, then the descriptor figures of
flatten_srt_kernel<3, false, false>: VGPRs, occupancy, private segment, spilled SGPRs, static v_readlane / v_writelane."""
import collections
import re
import sys

SRT = "flatten_srt_kernelILi3ELb0ELb0EE"


def kernels(path):
    """{kernel symbol: Counter((opcode, policy) -> n)} and {symbol: descriptor figures}"""
    ops, desc = {}, {}
    cur, body = None, False
    for line in open(path, errors="replace"):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body = m.group(1), True
            ops[cur] = collections.Counter()
            desc[cur] = collections.Counter()
            continue
        if cur is None:
            continue
        s = line.strip()
        if line.startswith(".Lfunc_end"):
            body = False
        m = re.match(r"(buffer_\w+|global_\w+|flat_\w+|scratch_\w+)\s", s)
        if m and body:
            code = s.split(";")[0].split()
            pol = " ".join(b for b in ("sc0", "sc1", "nt") if b in code) or "-"
            ops[cur][(m.group(1), pol)] += 1
        for name in ("v_readlane_b32", "v_writelane_b32"):
            if body and s.startswith(name):
                desc[cur][name] += 1
        m = re.match(r"; (NumVgprs|Occupancy|ScratchSize|SGPRBlocks|NumSgprs|sgpr spill count|vgpr spill count): (\d+)", s, re.I)
        if m:
            desc[cur][m.group(1)] = int(m.group(2))
    return ops, desc


def main():
    base_ops, base_desc = kernels(sys.argv[1])
    total = sum(sum(c.values()) for c in base_ops.values())
    print(f"{sys.argv[1]}: {len(base_ops)} kernels, {total} memory instructions; policy bits set: "
          f"{sum(n for c in base_ops.values() for (o, p), n in c.items() if p != '-')}")
    srt = [k for k in base_desc if SRT in k]
    print("  srt<3,0,0>:", {k: dict(base_desc[k]) for k in srt})
    for path in sys.argv[2:]:
        ops, desc = kernels(path)
        print(path)
        assert set(ops) == set(base_ops), "kernel sets differ"
        for k in sorted(ops):
            if ops[k] != base_ops[k]:
                by_op = lambda c: collections.Counter({o: sum(n for (o2, p), n in c.items() if o2 == o) for (o, _) in c})
                same = by_op(ops[k]) == by_op(base_ops[k])
                moved = {f"{o} [{p}]": ops[k].get((o, p), 0) - base_ops[k].get((o, p), 0) for (o, p) in sorted(set(ops[k]) | set(base_ops[k]))
                         if ops[k].get((o, p), 0) != base_ops[k].get((o, p), 0)}
                print(f"  {k[:70]}: opcode counts {'equal' if same else 'DIFFER'}; {moved}")
        for k in srt:
            print(f"  srt<3,0,0>: {dict(desc[k])}{'' if desc[k] == base_desc[k] else '   <-- differs from the first file'}")


if __name__ == "__main__":
    main()
