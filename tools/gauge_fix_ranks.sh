#!/bin/bash
# Two ranks of tools/gauge_fix_ranks.py on one GPU (both on device 0, file-based rehearsal transport, as tools/gauge_md_ranks.sh), each
# under its own time limit; a rank that fails ends the script with its status.  usage: tools/gauge_fix_ranks.sh inputs.npz outdir
IN=$1; OUT=$2; N=2
export MASTER_ADDR=127.0.0.1 MASTER_PORT=$((20000 + $$ % 20000)) WORLD_SIZE=$N QUDA_AMD_FORCE_DEVICE=0
export QUDA_AMD_TRANSPORT=shm QUDA_AMD_SHM_DIR=$(mktemp -d /dev/shm/quda_amd_XXXXXX)
cd "$(dirname "$0")/.."
pids=()
for r in $(seq 0 $((N-1))); do
  RANK=$r LOCAL_RANK=$r timeout -k 10 240 python3 -u tools/gauge_fix_ranks.py "$IN" "$OUT" > "$OUT/rank$r.log" 2>&1 &
  pids+=($!)
done
rc=0
for p in "${pids[@]}"; do wait $p || rc=$?; done
rm -rf "$QUDA_AMD_SHM_DIR"
exit $rc
