#!/bin/bash
# tools/kasm.sh [--hash] <file.hip> [extra flags]: device-only assembly of one translation unit of csrc/ into
# $DV_KASM_OUT (default /tmp)/<name>.s and the register / spill summary of every kernel in it (CPU only; hipcc
# cross-compiles gfx950).  DV_KASM_CSRC names another checkout's csrc/ directory (comparing against a parent commit).
# --hash: per kernel also the instruction count and a hash of its instruction stream with block labels normalised
# (.LBB<fn>_<n> -> .LBB_<n>), comments and assembler directives dropped, and the namespace qualifier stripped from the
# demangled name -- equal lines for two commits mean the same device code wherever the kernel lives.
mode=regs
if [ "$1" = "--hash" ]; then mode=hash; shift; fi
f=$1; shift
n=$(basename "$f" .hip)
ROOT=$(cd "$(dirname "$0")/.." && pwd)
CSRC=${DV_KASM_CSRC:-$ROOT/deepvariant_amd/csrc}
OUT=${DV_KASM_OUT:-/tmp}
cd "$CSRC" || exit 1
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -I"$CSRC/../../include" -I. --cuda-device-only -S $n.hip -o "$OUT/$n.s" "$@" 2>&1 | grep -E "error"
python3 - "$OUT/$n.s" $mode <<'P'
import hashlib, re, subprocess, sys
t = open(sys.argv[1]).read()
meta = {}
for m in re.finditer(r'\.group_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.name:\s+(\S+)\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n\s+\.sgpr_spill_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)\n\s+\.vgpr_spill_count:\s+(\d+)', t):
    meta[m.group(2)] = m.groups()
if sys.argv[2] == 'regs':
    for name, g in meta.items():
        print('%-90s scratch %4s  sgpr %3s (spill %s)  vgpr %3s (spill %s)' % (name[:90], g[2], g[3], g[4], g[5], g[6]))
    sys.exit(0)
plain = subprocess.run(['c++filt'] + list(meta), capture_output=True, text=True).stdout.split('\n')
rows = []
for (name, g), dem in zip(meta.items(), plain):
    body = re.search(r'^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:' % re.escape(name), t, re.S | re.M).group(1)
    ins = []
    for line in body.split('\n'):
        line = re.sub(r'\.LBB\d+_', '.LBB_', line.split(';')[0]).strip()
        if line and not (line.startswith('.') and not line.startswith('.LBB_')):
            ins.append(line)
    if dem == name:   # a type c++filt does not know (_Float16): the last length-prefixed part of the nested name
        at = 3
        while name[at].isdigit():
            n_len = re.match(r'\d+', name[at:]).group(0)
            dem = name[at + len(n_len):at + len(n_len) + int(n_len)] + '('
            at += len(n_len) + int(n_len)
    dem = re.sub(r'\(anonymous namespace\)::|dv::\w+::', '', dem)
    dem = re.sub(r'^void ', '', dem).rsplit('(', 1)[0]
    rows.append('%-64s insts %5d  %s  vgpr %3s sgpr %3s spill %s/%s scratch %s lds %s' % (
        dem, sum(1 for i in ins if not i.startswith('.LBB_')), hashlib.sha256('\n'.join(ins).encode()).hexdigest()[:16],
        g[5], g[3], g[6], g[4], g[2], g[0]))
print('\n'.join(sorted(rows)))
P
