#!/usr/bin/env python3
"""Accumulation-register discipline of the parked chain kernels (chain_factor_solve_qw16<..., PARK>, chain_qw16.hpp).

  check_park_regs.py <listing.s> [kernel name substring ...]

The kernel keeps the spill image of its first KEEP nodes in banks of 13 accumulation registers, a[0] .. a[13 KEEP - 1],
between its two sweeps.  The banks are moved only by asm blocks that stand between the comment markers
`sip_park_begin` / `sip_park_end`; nothing tells the compiler that their contents live on between two blocks.  What
keeps them safe is that the compiler takes the registers it spills to from those no asm block of the function names.
This check reads the register NAMES of the listing and holds the build to that, per kernel that has the markers:

  * the registers named between the markers are exactly a[0] .. a[13 K - 1] for some K >= 1 (the banks);
  * no instruction outside the markers names a register of the banks (the compiler's own spill registers lie above);
  * the kernel uses no scratch (a spill to memory would shift every counted vmcnt wait);
  * the descriptor's totals fit the register file of one wavefront per SIMD: next_free_vgpr <= 512, accum_offset <=
    256, and accum_offset + (highest accumulation register named + 1) <= next_free_vgpr.

Prints one line per kernel (K, the compiler's own accumulation registers, the totals); exit status 1 on a violation."""
import re
import sys

BANK = 13
AREG = re.compile(r"(?<![\w.$])a(?:(\d+)|\[([^\]]+)\])(?![\w(])")


def agprs(line):
    """Accumulation-register numbers an instruction line names: a7, a[7], a[26+3], a[4:7]."""
    code = line.split(";")[0]
    if not code.strip() or code.strip().startswith("."):
        return set()
    out = set()
    for m in AREG.finditer(code):
        if m.group(1) is not None:
            out.add(int(m.group(1)))
            continue
        lo, _, hi = m.group(2).partition(":")
        first = sum(int(t, 0) for t in lo.split("+"))  # (the compiler prints large immediates in hex)
        last = sum(int(t, 0) for t in hi.split("+")) if hi else first
        out.update(range(first, last + 1))
    return out


def kernels(text):
    """(name, body lines, descriptor text) of every kernel of a listing."""
    desc = {m.group(1): m.group(2) for m in
            re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)}
    lines = text.split("\n")
    for name, d in desc.items():
        start = lines.index(name + ":") if name + ":" in lines else next(
            i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
        yield name, lines[start + 1:end], d


def check_kernel(name, body, desc):
    """(problems, summary) of one kernel; summary is None for a kernel without the markers."""
    inside, outside, depth, problems = set(), set(), 0, []
    for ln in body:
        if "sip_park_begin" in ln:
            depth += 1
            continue
        if "sip_park_end" in ln:
            depth -= 1
            continue
        (inside if depth > 0 else outside).update(agprs(ln))
    if depth != 0:
        problems.append("unbalanced sip_park_begin / sip_park_end markers")
    if not inside:
        return problems, None
    keep = (max(inside) + 1) // BANK
    if inside != set(range(BANK * keep)) or keep < 1:
        problems.append("the marked blocks name %s, not whole banks a[0] .. a[13 K - 1]" % sorted(inside)[:8])
    clash = sorted(outside & set(range(max(inside) + 1)))
    if clash:
        problems.append("registers of the banks named outside the markers: " + ", ".join("a%d" % r for r in clash[:12]))

    def field(key):
        m = re.search(r"\.amdhsa_%s (\d+)" % key, desc)
        return int(m.group(1)) if m else None
    scratch, nfree, accum = field("private_segment_fixed_size"), field("next_free_vgpr"), field("accum_offset")
    if scratch != 0:
        problems.append("scratch: private_segment_fixed_size %s" % scratch)
    top = max(inside | outside) + 1
    if nfree is None or accum is None or nfree > 512 or accum > 256 or accum + top > nfree:
        problems.append("register totals: next_free_vgpr %s, accum_offset %s, accumulation registers %d" % (nfree, accum, top))
    return problems, {"keep": keep, "own": len(outside), "own_lowest": min(outside) if outside else None,
                      "next_free_vgpr": nfree, "accum_offset": accum}


def main(argv):
    text = open(argv[1]).read()
    wanted, bad, seen = argv[2:], 0, 0
    for name, body, desc in kernels(text):
        if wanted and not any(w in name for w in wanted):
            continue
        problems, summary = check_kernel(name, body, desc)
        if summary is None and not problems:
            continue
        seen += 1
        print("%s: %s" % (name, summary))
        for p in problems:
            bad += 1
            print("   [" + p + "]")
    print("%d parked kernel(s), %d problem(s)" % (seen, bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
