#!/bin/bash
# Register tables of k_resample_pk: every form of the library (8 accumulator counts x {1024, 768, 512, 256} threads at
# groups of five, and the default size at groups of four) instantiated explicitly with one body, compiled alone for
# gfx950 with the library's flags, the figures of -Rpass-analysis=kernel-resource-usage one line per form.
# Usage: tools/pk_regs.sh true|false [all]   (the second body | the present body) -- needs no GPU; about two minutes.
# The second body is compiled for the forms the library gives it (pk_pipelined: 1024 threads, up to 20 accumulators);
# with `all` for every form, also for those that pk_pipelined leaves on the present body.
set -e
cd "$(dirname "$0")/.."
BODY=${1:-true}
ALL=${2:-}
T=$(mktemp -d)
{
  echo '#include "kernels.hip.h"'
  echo 'namespace bmm {'
  for kt in 4 8 12 16 20 24 28 32; do
    for nt in 1024 768 512 256; do
      if [ $BODY = true ] && [ -z "$ALL" ] && { [ $nt -ne 1024 ] || [ $kt -gt 20 ]; }; then continue; fi
      echo "template __global__ void k_resample_pk<$kt, $nt, 5, $BODY>(ChainParams, ResampleArgs);"
    done
    if [ $kt -le 20 ]; then nt=1024; else nt=768; fi
    if [ $BODY = true ] && [ -z "$ALL" ] && [ $kt -gt 20 ]; then continue; fi
    echo "template __global__ void k_resample_pk<$kt, $nt, 4, $BODY>(ChainParams, ResampleArgs);"
  done
  echo '}'
} > $T/pk_forms.hip
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -amdgpu-sched-strategy=iterative-ilp \
  -Ibmm-mcmc_amd/csrc --cuda-device-only -S -Rpass-analysis=kernel-resource-usage -o $T/pk_forms.s $T/pk_forms.hip 2>&1 | python3 -c "
import re, sys
cur, rows = None, {}
for l in sys.stdin:
    if 'error' in l: print(l.rstrip())
    m = re.search(r'remark:\s+(.*?) \[-Rpass', l)
    if not m: continue
    t = m.group(1).strip()
    if t.startswith('Function Name:'): cur = t.split(': ')[1]; rows[cur] = {}
    elif cur and ':' in t:
        k, v = t.split(':', 1); rows[cur][k.strip()] = v.strip()
for n, r in rows.items():
    m = re.search(r'k_resample_pkILi(\d+)ELi(\d+)ELi(\d+)ELb', n)
    if m: print('accumulators %s threads %s group width %s VGPRs %s SGPR spill slots %s VGPR spills %s scratch bytes/lane %s waves/SIMD by registers %s' % (
        m.group(1), m.group(2), m.group(3), r.get('VGPRs'), r.get('SGPRs Spill'), r.get('VGPRs Spill'), r.get('ScratchSize [bytes/lane]'), r.get('Occupancy [waves/SIMD]')))
"
rm -rf $T
