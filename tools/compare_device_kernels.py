#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the device code of two builds of libvqs_hip.so: the evidence that a host-side change edited no kernel.

  compare_device_kernels.py A.so B.so [OUT.md]

For every kernel symbol (bench.device_kernels): machine code and kernel descriptor, the descriptor with its entry-offset field zeroed as
bench.gemm_kernels_hash does (where the linker put the code, not what it is).  Prints / writes the counts, the symbols only in A, only in B
and the symbols present in both that differ; exit status 1 when a symbol of both differs or B has a symbol A lacks."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def kernels(path):
    return {n: (code, kd[:16] + b"\0" * 8 + kd[24:]) for n, (code, kd) in bench.device_kernels(path).items()}


def main(a, b, out=None):
    ka, kb = kernels(a), kernels(b)
    gone, new = sorted(set(ka) - set(kb)), sorted(set(kb) - set(ka))
    differ = sorted(n for n in set(ka) & set(kb) if ka[n] != kb[n])
    lines = [f"A: {len(ka)} kernels, B: {len(kb)} kernels", f"in both: {len(set(ka) & set(kb))}, of which {len(differ)} differ (machine code or descriptor)",
             f"only in A: {len(gone)}", *("  " + n for n in gone), f"only in B: {len(new)}", *("  " + n for n in new),
             *("DIFFERS: " + n for n in differ)]
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    if out:
        with open(out, "w") as f:
            f.write("```\n" + text + "```\n")
    return 1 if differ or new else 0


if __name__ == "__main__":
    sys.exit(main(*sys.argv[1:4]))
