#!/bin/bash
# Does the DAG's HBM operand stream cost clock?  The DAG's accumulation loop in isolation
# (tools/probe/accum_probe config 9: 128 x 128 tiles, 4 waves, the ring of five 16-deep LDS-DMA
# stages), with its operands held in L2 (mode 2: K wrapped at 1024 rows, 2 MB of operands), with
# four workgroups per column panel (mode 1: ~0.6 TB/s of distinct bytes, the rest cache re-reads
# -- what round 4 took for the HBM stream) and with a column panel per workgroup out of a 9-GB
# buffer (mode 3: ~2.3 TB/s of distinct bytes, the job's load).  TF/s and in-kernel clock after
# 3 s of launches each, modes alternating; then effective clock = GRBM_GUI_ACTIVE / 8 XCDs /
# dispatch duration and MFMA busy = SQ_VALU_MFMA_BUSY_CYCLES / (clock cycles x 1024 SIMDs), one
# --pmc pass per counter and mode.
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=$ROOT/gpurun_out/clock_stream
rm -rf $OUT && mkdir -p $OUT
cd /tmp && export TMPDIR=/tmp
for mode in 2 1 3 2 1 3; do
  timeout -k 10 120 $ROOT/tools/probe/accum_probe 32768 40 9 $mode 3 >> $OUT/probe.txt 2>&1 || exit 1
done
for mode in 2 1 3; do
  for c in SQ_VALU_MFMA_BUSY_CYCLES GRBM_GUI_ACTIVE; do
    timeout -s KILL 240 rocprofv3 --pmc $c --output-format csv -d $OUT/pmc_m${mode}_$c -o p -- $ROOT/tools/probe/accum_probe 32768 20 9 $mode 1 > $OUT/pmc_m${mode}_$c.txt 2>&1 || exit 1
  done
done
echo clock_stream done
