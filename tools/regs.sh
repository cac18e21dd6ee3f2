#!/bin/bash
# Register / scratch / occupancy / LDS summary of every kernel of every HIP unit the Makefile builds (its CSRC list; cross-compiled, no GPU
# needed). Extra flags: EXTRA=-D...   Another tree: PKG=<its thu-acg-f2024-path-tracer_amd>.   One unit: UNITS=csrc/pt_k2.hip
#   tools/regs.sh              the table, one line per kernel, headed by the unit's name
#   tools/regs.sh --isa DIR    also writes the gfx950 assembly of every kernel and every non-inlined device function, in the order of their
#                              symbols, to DIR/<unit>.s, normalised — comments stripped, the labels that carry the function's position in its
#                              unit (.LBB<N>_, .Lfunc_begin<N> / _end<N>, .Ltmp<N>, ...) renumbered, the kernel's descriptor appended — and
#                              DIR/MANIFEST: "<sha256> <kernel|func> <symbol> <unit>" sorted by symbol. Two trees hold the same code when
#                              `cut -d' ' -f1-3 MANIFEST | sort -u` of both are equal (the order of functions and units does not enter).
#                              And DIR/MANIFEST.anon: "<sha256> <kernel|func> <unit>" of the same text with every occurrence of the
#                              function's own symbol replaced by one token. Two trees hold the same code up to the renaming of functions
#                              (a template's arguments respelt) when `cut -d' ' -f1-2 MANIFEST.anon | sort` of both are equal.
set -e
ISA=
[ "$1" = "--isa" ] && { ISA=$(mkdir -p "$2" && cd "$2" && pwd); rm -f "$ISA"/*.s "$ISA"/MANIFEST "$ISA"/MANIFEST.anon; }
cd "${PKG:-$(dirname "$0")/../thu-acg-f2024-path-tracer_amd}"
UNITS=${UNITS:-$(sed -n 's/^CSRC *= *//p' Makefile | tr ' ' '\n' | grep '\.hip$')}
TMP=$(mktemp -d)
trap 'rm -rf "$TMP"' EXIT
for u in $UNITS; do   # the units compile side by side; the tables come out in the Makefile's order
  n=$(basename "$u" .hip)
  /opt/rocm/bin/hipcc --offload-arch=gfx950 -std=c++17 -O3 -ffp-contract=off -fPIC $EXTRA --cuda-device-only -S "$u" -o "$TMP/$n.s" \
      -Rpass-analysis=kernel-resource-usage > "$TMP/$n.log" 2>&1 &
done
wait
for u in $UNITS; do
  n=$(basename "$u" .hip)
  echo "== $n"
  [ -s "$TMP/$n.s" ] || { cat "$TMP/$n.log"; exit 1; }
  grep -E "Function Name|VGPRs:|ScratchSize|Occupancy|LDS Size" "$TMP/$n.log" | sed -e 's/.*remark: //' -e 's/ \[-Rpass.*//' | paste - - - - - \
   | sed -e 's/Function Name: _ZN2pt//' -e 's/    */ /g' | cut -c1-230
done
[ -z "$ISA" ] && exit 0
python3 - "$ISA" "$TMP"/*.s <<'EOF'
import hashlib, os, re, sys
out, manifest, anon = sys.argv[1], [], []
label = re.compile(r"\.L([A-Za-z_]+?)(\d+)(_\d+)?\b")
for path in sys.argv[2:]:
    unit = os.path.basename(path)[:-2]
    lines = [l.split(";")[0].rstrip() for l in open(path)]
    lines = [l for l in lines if l.strip()]
    funcs = {l.split()[1].split(",")[0] for l in lines if l.lstrip().startswith(".type") and l.endswith("@function")}
    kernels = {l.split()[1] for l in lines if l.lstrip().startswith(".amdhsa_kernel")}
    text, cur = {}, None
    for l in lines:
        if cur is None and l.endswith(":") and l[:-1] in funcs:
            cur = l[:-1]
            text[cur] = []
        if cur is not None:
            text[cur].append(l)
            if l.startswith(".Lfunc_end"):
                cur = None
        if l.lstrip().startswith(".amdhsa_kernel"):
            cur = l.split()[1]
            text.setdefault(cur, [])
        elif l.lstrip().startswith(".end_amdhsa_kernel"):
            cur = None
    per_unit = open(os.path.join(out, unit + ".s"), "w")
    for sym, body in sorted(text.items()):
        tmp = {}
        def renumber(m):
            if m.group(3):                       # .LBB<N>_<k>: N is the function's index in its unit
                return ".L%s_%s" % (m.group(1), m.group(3))
            if m.group(1).startswith("func_"):   # .Lfunc_begin<N>, .Lfunc_end<N>
                return ".L" + m.group(1)
            return ".L%s#%d" % (m.group(1), tmp.setdefault(m.group(0), len(tmp)))   # .Ltmp<N>: by first appearance
        norm = "\n".join(label.sub(renumber, l) for l in body) + "\n"
        per_unit.write("== %s\n%s" % (sym, norm))
        kind = "kernel" if sym in kernels else "func"
        manifest.append("%s %s %s %s" % (hashlib.sha256(norm.encode()).hexdigest(), kind, sym, unit))
        anon.append("%s %s %s" % (hashlib.sha256(norm.replace(sym, "@SELF").encode()).hexdigest(), kind, unit))
manifest.sort(key=lambda m: m.split()[2:])
open(os.path.join(out, "MANIFEST"), "w").write("\n".join(manifest) + "\n")
open(os.path.join(out, "MANIFEST.anon"), "w").write("\n".join(sorted(anon)) + "\n")
print("%d kernels, %d device functions -> %s/MANIFEST" % (sum(" kernel " in m for m in manifest), sum(" func " in m for m in manifest), out))
EOF
