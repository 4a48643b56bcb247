# SQ counters (one pass of eight) of the kernel round 5 was about: the weight-stationary forward kernel with the ReLU per
# A fragment (shipped).  The ReLU-sweep and K-split-across-workgroups arms of that round were removed from the tree after
# 6754f7c; their counters are in profiles/r05_sq_counters_conv.json.
# usage (GPU box): bash tools/sq_round5.sh && python tools/summarize_sq.py r05 gpurun_out/sq5_*
set -e
R=$GRAFT_REPO_ROOT
export TMPDIR=/tmp
cd $R
C="SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES SQ_WAVE_CYCLES SQ_WAIT_ANY SQ_WAIT_INST_ANY SQ_ACTIVE_INST_ANY SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE"
rocprofv3 --pmc $C --kernel-trace --output-format csv -d $R/gpurun_out/sq5_ws64_perfragment -- python3 tools/ws_probe.py > /dev/null 2> $R/gpurun_out/sq5_ws64_perfragment.err
echo "sq ws64 per-fragment done"
find $R/gpurun_out/sq5_* -name "*kernel_trace.csv" -delete || true
