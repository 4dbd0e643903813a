#!/usr/bin/env python3
"""Registers, LDS and scratch of every k_left_to_right instantiation (and of
k_ltr_reduce), from the kernel descriptors of the built library's gfx950 code
object, as heldout_isa.py reads k_doc_completion's.  Exits 1 if one uses
scratch.

  python tools/left_to_right_isa.py [path/to/liblda_mi355x.so]
"""
import os
import re
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from heldout_isa import describe  # noqa: E402
from ldagibbssampling_amd import capi, codeobj  # noqa: E402


def rows(lib: str) -> list:
    """[(kernel, C or None, text bytes, descriptor fields)], by C."""
    ks = codeobj.kernels(codeobj.device_code_object(lib))
    pre, red = codeobj.mangled_prefix("k_left_to_right"), codeobj.mangled_prefix("k_ltr_reduce")
    out = []
    for name, (text, kd) in ks.items():
        m = re.match(re.escape(pre) + r"ILi(\d+)E", name)
        if m and kd:
            out.append(("k_left_to_right", int(m.group(1)), len(text), describe(kd)))
        elif name.startswith(red) and kd:
            out.append(("k_ltr_reduce", None, len(text), describe(kd)))
    return sorted(out, key=lambda r: (r[1] is None, r[1] or 0))


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else capi.LIB_PATH
    found = rows(lib)
    if not any(r[0] == "k_left_to_right" for r in found):
        sys.exit(f"{lib}: no k_left_to_right kernel")
    bad = False
    print("| kernel | C | arch VGPRs | VGPRs + AGPRs | LDS B | scratch B | text B |")
    print("|---|---|---|---|---|---|---|")
    for kernel, C, size, d in found:
        print(f"| {kernel} | {'' if C is None else C} | {d['arch_vgprs']} | {d['vgprs_total']} | {d['lds_bytes']} | "
              f"{d['scratch_bytes']} | {size} |")
        bad |= d["scratch_bytes"] != 0 or d["scratch_enabled"]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
