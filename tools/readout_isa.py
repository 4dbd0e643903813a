#!/usr/bin/env python3
"""Registers, LDS and scratch of the readout kernels (k_top_words_slab,
k_top_words_merge, k_doc_top_topics, k_doc_counts), from the kernel
descriptors of the built library's gfx950 code object (walked as
ldagibbssampling_amd/codeobj.py walks it; the descriptor fields as
tools/heldout_isa.py reads them).  The slab kernel's and the document
kernels' LDS is dynamic (512 n bytes; 16 Kp bytes), so the descriptor shows
only the static part.  Exits 1 if a kernel uses scratch.

  python tools/readout_isa.py [path/to/liblda_mi355x.so]
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from ldagibbssampling_amd import capi, codeobj  # noqa: E402
from heldout_isa import describe  # noqa: E402

KERNELS = ["k_top_words_slab", "k_top_words_merge", "k_doc_top_topics", "k_doc_counts"]


def main():
    lib = sys.argv[1] if len(sys.argv) > 1 else capi.LIB_PATH
    ks = codeobj.kernels(codeobj.device_code_object(lib))
    bad = False
    print("| kernel | arch VGPRs | VGPRs + AGPRs | static LDS B | scratch B | text B |")
    print("|---|---|---|---|---|---|")
    for k in KERNELS:
        pre = codeobj.mangled_prefix(k)
        found = [(name, v) for name, v in ks.items() if name.startswith(pre) and v[1]]
        if not found:
            sys.exit(f"{lib}: no {k} kernel")
        for name, (text, kd) in found:
            d = describe(kd)
            print(f"| {k} | {d['arch_vgprs']} | {d['vgprs_total']} | {d['lds_bytes']} | {d['scratch_bytes']} | {len(text)} |")
            bad |= d["scratch_bytes"] != 0 or d["scratch_enabled"]
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
