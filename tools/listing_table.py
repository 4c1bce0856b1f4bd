#!/usr/bin/env python3
"""tools/listing_table.py LISTING.s [--dump KERNEL]  — the table of profiles/*loop_summary.md from a device listing

The listing is pt_lib.hip compiled with the Makefile's FLAGS plus `--cuda-device-only -S`.  For every traversal kernel: registers, spills,
scratch, LDS from the kernel's metadata, and for every innermost loop that holds the five node loads (five consecutive
`global_load_dwordx4`) the instructions and VALU instructions of all blocks the compiler marks as belonging to that loop, cold blocks
included.  --dump prints those loops' blocks of one kernel (substring of the demangled name) for a hand walk."""
import re
import subprocess
import sys

WANTED = ("k_trace8_vis", "k_trace8<", "k_path_loop<", "k_path_loop_views<")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.split("\n")
    return dict(zip(names, out))


def kernels(text):
    """{mangled: [lines]} of every function body"""
    out, cur = {}, None
    for ln in text.split("\n"):
        m = re.match(r"^(_Z\w+):\s", ln)
        if m:
            cur = m.group(1)
            out[cur] = []
        elif cur and ln.startswith(".Lfunc_end"):
            cur = None
        elif cur:
            out[cur].append(ln)
    return out


def blocks(lines):
    """[(label, header or None, is_header, [instructions])]"""
    out = []
    cur = ["entry", None, False, []]
    for i, ln in enumerate(lines):
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):", ln)
        if m:
            out.append(tuple(cur))
            label = m.group(1).replace("; %bb.", "bb.")
            hdr = re.search(r"in Loop: Header=(BB\d+_\d+)", ln)
            own = "Loop Header" in ln or (i + 1 < len(lines) and "Loop Header" in lines[i + 1] and not re.match(r"^(\.LBB|; %bb)", lines[i + 1]))
            # a header's own line reads "=>This (Inner) Loop Header", possibly on the continuation lines after "Parent Loop"
            j = i
            while not own and j + 1 < len(lines) and lines[j + 1].startswith("  ") and lines[j + 1].lstrip().startswith(";"):
                j += 1
                own = "Loop Header" in lines[j]
            cur = [label, hdr.group(1) if hdr else (label[2:] if own and label.startswith(".L") else None), own, []]
            continue
        s = ln.strip()
        if s and not s.startswith((";", ".")) and not s.endswith(":"):
            cur[3].append(s.split(";")[0].strip())
    out.append(tuple(cur))
    return out


def node_loops(bl):
    """headers of the innermost loops that hold five consecutive global_load_dwordx4"""
    hs = []
    for label, hdr, own, ins in bl:
        run = 0
        for s in ins:
            run = run + 1 if s.startswith("global_load_dwordx4") else (run if s.startswith("s_waitcnt") else 0)
            if run == 5 and hdr and hdr not in hs:
                hs.append(hdr)
    return hs


def main():
    text = open(sys.argv[1]).read()
    dump = sys.argv[3] if len(sys.argv) > 3 and sys.argv[2] == "--dump" else None
    ks = kernels(text)
    dm = demangle(list(ks))
    meta = {}
    for m in re.finditer(r"  - \.agpr_count:.*?(?=\n  - \.agpr_count:|\namdhsa\.target)", text, re.S):
        f = dict(re.findall(r"\.(name|sgpr_count|vgpr_count|sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size|group_segment_fixed_size):\s+(\S+)", m.group(0)))
        meta[f["name"]] = f
    print("| kernel | VGPR | SGPR | SGPR spills | VGPR spills | scratch, B | LDS, B | instructions | loops: instructions | loops: VALU | loops: LDS accesses |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for k, lines in ks.items():
        name = dm[k].split("(")[0].replace("void ", "")
        if not name.startswith(WANTED) or k not in meta:
            continue
        bl = blocks(lines)
        total = sum(len(b[3]) for b in bl)
        cols = [[], [], []]
        for h in node_loops(bl):
            ins = [s for b in bl if b[1] == h for s in b[3]]
            cols[0].append(str(len(ins)))
            cols[1].append(str(sum(s.startswith("v_") for s in ins)))
            cols[2].append(str(sum(s.startswith("ds_") for s in ins)))
            if dump and dump in name:
                print(f"==== {name}: loop {h}", file=sys.stderr)
                for b in bl:
                    if b[1] == h:
                        print(f"{b[0]}:", file=sys.stderr)
                        for s in b[3]:
                            print("    " + s, file=sys.stderr)
        f = meta[k]
        print(f"| `{name}` | {f['vgpr_count']} | {f['sgpr_count']} | {f['sgpr_spill_count']} | {f['vgpr_spill_count']} | {f['private_segment_fixed_size']} | "
              f"{f['group_segment_fixed_size']} | {total} | {' + '.join(cols[0])} | {' + '.join(cols[1])} | {' + '.join(cols[2])} |")


if __name__ == "__main__":
    main()
