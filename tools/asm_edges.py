#!/usr/bin/env python3
"""Kernel-by-kernel comparison of two device assemblies of one .hip source (CPU only), with the counts that describe a kernel's EDGES:
what stands between entry and the first LDS-DMA, and what stands behind the last MFMA.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC --cuda-device-only -S igemm.hip -o tree.s      (and the same of the parent)
  python tools/asm_edges.py parent.s tree.s [substring ...]

Per kernel: instruction lines (labels numbered per kernel, comments and directives dropped), v_mfma count, LDS / scratch / register
lines of the .amdhsa_ block; in front of the first `buffer_load ... lds`: global_load / buffer_load (not lds) / s_waitcnt vmcnt /
s_load counts and the line of that first DMA; behind the last v_mfma: lines, ds_bpermute, s_waitcnt, global / buffer stores."""
import re
import subprocess
import sys

AMDHSA = ("group_segment_fixed_size", "private_segment_fixed_size", "next_free_vgpr", "accum_offset")


def kernels(path):
    body, meta, cur, hsa = {}, {}, None, None
    for raw in open(path):
        line = raw.split(";")[0].rstrip()
        s = line.strip()
        if not s:
            continue
        m = re.match(r"^(_Z\w+):", s)
        if m and cur is None:
            cur = m.group(1)
            body[cur] = []
            continue
        if s.startswith(".amdhsa_kernel "):
            hsa = s.split()[1]
            meta[hsa] = {}
            continue
        if s == ".end_amdhsa_kernel":
            hsa = None
            continue
        if hsa is not None:
            k, _, v = s.partition(" ")
            k = k.replace(".amdhsa_", "")
            if k in AMDHSA:
                meta[hsa][k] = v.strip()
            continue
        if cur is not None:
            if s.startswith(".Lfunc_end"):
                cur = None
                continue
            if s.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", s):
                continue
            body[cur].append(s)
    out = {}
    for name, lines in body.items():
        if name not in meta:
            continue
        labels = {}
        norm = []
        for s in lines:
            def sub(m):
                return labels.setdefault(m.group(0), ".L%d" % len(labels))
            norm.append(re.sub(r"\.LBB\d+_\d+", sub, s))
        out[name] = (norm, meta[name])
    return out


def edges(lines):
    ins = [s for s in lines if not s.endswith(":")]
    is_dma = lambda s: s.startswith("buffer_load") and s.endswith(" lds")
    first = next((i for i, s in enumerate(ins) if is_dma(s)), None)
    head = ins[:first] if first is not None else []
    last = max((i for i, s in enumerate(ins) if s.startswith("v_mfma")), default=None)
    tail = ins[last + 1:] if last is not None else []
    cnt = lambda seq, f: sum(1 for s in seq if f(s))
    return {
        "lines": len(ins),
        "mfma": cnt(ins, lambda s: s.startswith("v_mfma")),
        "first_dma": first,
        "head_gload": cnt(head, lambda s: s.startswith("global_load")),
        "head_bload": cnt(head, lambda s: s.startswith("buffer_load")),
        "head_vmcnt": cnt(head, lambda s: s.startswith("s_waitcnt") and "vmcnt" in s),
        "head_sload": cnt(head, lambda s: s.startswith("s_load")),
        "head_lgkm": cnt(head, lambda s: s.startswith("s_waitcnt") and "lgkmcnt" in s),
        "tail_lines": len(tail),
        "tail_bperm": cnt(tail, lambda s: s.startswith("ds_bpermute")),
        "tail_dpp": cnt(tail, lambda s: "row_ror" in s),
        "tail_wait": cnt(tail, lambda s: s.startswith("s_waitcnt")),
        "tail_store": cnt(tail, lambda s: s.startswith("global_store") or s.startswith("buffer_store")),
        "bperm": cnt(ins, lambda s: s.startswith("ds_bpermute")),
    }


def fmt(e, m):
    return ("lines %d  mfma %d  lds %s  scratch %s  vgpr %s/%s | entry..first DMA (line %s): global_load %d  buffer_load %d  vmcnt waits %d  s_load %d  "
            "lgkmcnt waits %d | behind the last MFMA: lines %d  ds_bpermute %d  row_ror %d  s_waitcnt %d  stores %d | ds_bpermute in all %d" %
            (e["lines"], e["mfma"], m.get("group_segment_fixed_size"), m.get("private_segment_fixed_size"), m.get("next_free_vgpr"), m.get("accum_offset"),
             e["first_dma"], e["head_gload"], e["head_bload"], e["head_vmcnt"], e["head_sload"], e["head_lgkm"], e["tail_lines"], e["tail_bperm"], e["tail_dpp"],
             e["tail_wait"], e["tail_store"], e["bperm"]))


def alloc_step(v):  # gfx950 allocates vector registers in blocks of 8
    return (int(v) + 7) // 8 * 8


if __name__ == "__main__":
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    pats = sys.argv[3:]
    names = sorted(set(a) | set(b))
    dem = dict(zip(names, subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")))
    same = 0
    bad = []
    for n in names:
        d = re.sub(r"\(IgemmP\)$", "", re.sub(r"^void ", "", dem[n]))
        if pats and not any(p in d for p in pats):
            continue
        if n not in a or n not in b:
            print(("NEW   " if n in b else "GONE  ") + d)
            continue
        if a[n] == b[n]:
            same += 1
            continue
        ea, eb = edges(a[n][0]), edges(b[n][0])
        print("DIFF  " + d)
        print("      parent: " + fmt(ea, a[n][1]))
        print("      tree:   " + fmt(eb, b[n][1]))
        ma, mb = a[n][1], b[n][1]
        if ea["mfma"] != eb["mfma"] or ma.get("group_segment_fixed_size") != mb.get("group_segment_fixed_size") or int(mb.get("private_segment_fixed_size", 0)) > int(ma.get("private_segment_fixed_size", 0)) \
                or alloc_step(mb["next_free_vgpr"]) > alloc_step(ma["next_free_vgpr"]):
            bad.append(d)
    print("%d kernels identical (instruction lines and .amdhsa_ lines) of %d" % (same, len(names)))
    print("mfma count or LDS size changed, scratch or register allocation step above the parent's in: %s" % (", ".join(bad) if bad else "none"))
