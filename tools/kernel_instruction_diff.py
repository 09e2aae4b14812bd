#!/usr/bin/env python
"""Tooling: are the kernels of two builds of libirbpp_hip.so the same code?  Per kernel the static instruction count of
both libraries and whether the instruction streams (mnemonic + operands; addresses and branch-target offsets left
out) are identical -- the check a change that must leave existing kernels alone is held to.

    python tools/kernel_instruction_diff.py BEFORE.so AFTER.so [substring ...]

Kernels present in one library only are listed as such; with substrings only the kernels whose name contains one of
them are listed.  A kernel whose two streams have the same mnemonics and the same registers, instruction for instruction,
and differ in literal operands alone is reported as "immediates only", followed by the instructions concerned.
Exit code 1 if a kernel present in both differs.
"""
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from irbpp_amd import asmcheck  # noqa: E402


def streams(path):
    out = {}
    for name, ins in asmcheck.parse(asmcheck.disassemble(path)).items():
        out[name] = [(m, re.sub(r"\s+", " ", ops)) for _, m, ops, _ in ins]
    return out


LITERAL_RE = re.compile(r"(?<![\w\[:])(0x[0-9a-fA-F]+|\d+)(?![\w\]:])")


def masked(stream):
    """The stream with every literal operand (not a register number or range) blanked."""
    return [(m, LITERAL_RE.sub("#", ops)) for m, ops in stream]


def main(argv):
    before, after, want = streams(argv[1]), streams(argv[2]), argv[3:]
    differ = 0
    for name in sorted(set(before) | set(after)):
        if want and not any(w in name for w in want):
            continue
        a, b = before.get(name), after.get(name)
        if a is None or b is None:
            print(f"{name}: {'new' if a is None else 'gone'} ({len(b or a)} instructions)")
            continue
        same = a == b
        differ += not same
        if not same and len(a) == len(b) and masked(a) == masked(b):
            pairs = [(x, y) for x, y in zip(a, b) if x != y]
            print(f"{name}: {len(a)} -> {len(b)} instructions, immediates only ({len(pairs)} instructions)")
            for (m, x), (_, y) in pairs:
                print(f"    {m} {x}  ->  {y}")
            continue
        print(f"{name}: {len(a)} -> {len(b)} instructions, {'identical' if same else 'DIFFERENT'}")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv))
