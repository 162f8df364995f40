#!/bin/bash
# Regenerates the judged measurement artifacts on the GPU box (run through gpurun from the repo root):
#   $OUT/${ROUND}_bench_n1.json      the default bench line (roofline + cpu_baseline)
#   $OUT/${ROUND}_kernel_stats.txt   rocprofv3 --kernel-trace --stats summary of the same command (timed steps only)
#   $OUT/${ROUND}_pmc_counters.txt   rocprofv3 --pmc passes (one counter group per pass, no tracing) per kernel
#   $OUT/${ROUND}_kernel_table.txt   one line per kernel: HBM bytes, TB/s, MFMA busy %, VALU busy %, LDS conflict share (tools/pmc_table.py)
#   $OUT/gemm_nt_traffic.json   HBM bytes per k_gemm_nt launch from FETCH_SIZE/WRITE_SIZE (gfx950 correction applied)
# Copy them into profiles/ afterwards.
ROUND=${ROUND:-r06}
OUT=${OUT:-out}; export OUT; mkdir -p "$OUT"      # where the results go
cd /tmp && export TMPDIR=/tmp && cd $GRAFT_REPO_ROOT
if [ -z "$PMC_ONLY" ]; then
python3 bench.py --full 2> $OUT/${ROUND}_bench.err | tail -1 > $OUT/${ROUND}_bench_n1.json
timeout 400 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/_kt -o run -- python3 bench.py --full --steps 7 --warmup 3 --no-cpu-baseline --no-roofline --prewarm-s 0 --no-calibration > $OUT/_kt.log 2>&1
f=$(find $OUT/_kt -name "*kernel_trace.csv" | head -1)
{ echo "# rocprofv3 --kernel-trace --stats -- python3 bench.py --full --steps 7 --warmup 3 --no-cpu-baseline --no-roofline --prewarm-s 0 --no-calibration ; dispatches after the 6th k_soft_ce (3 warm-up steps dropped; kept: the 7 timed steps + the 6 forward+backward-only probe steps behind fwd_loss_bwd_only_ms_per_step)"; python3 tools/prof_summary.py $f --after k_soft_ce 6; } > $OUT/${ROUND}_kernel_stats.txt
rm -rf $OUT/_kt
fi
i=0
# FETCH_SIZE and WRITE_SIZE are derived metrics that do not fit one pass together ("exceeds the capabilities of the hardware",
# after which rocprofv3 aborts and hangs): one pass each, every pass under a hard timeout
for grp in "FETCH_SIZE" "WRITE_SIZE" "SQ_VALU_MFMA_BUSY_CYCLES SQ_BUSY_CYCLES GRBM_GUI_ACTIVE" "SQ_LDS_BANK_CONFLICT SQ_LDS_IDX_ACTIVE SQ_WAVE_CYCLES SQ_WAIT_ANY" "SQ_ACTIVE_INST_VALU SQ_INSTS_VALU"; do
  i=$((i+1))
  timeout 240 rocprofv3 --pmc $grp --output-format csv -d $OUT/_pmc/p$i -o run -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --prewarm-s 0 --no-calibration > $OUT/_pmc$i.log 2>&1
done
{ echo "# rocprofv3 --pmc <one group per pass> -- python3 bench.py --full --steps 2 --warmup 1 --no-cpu-baseline --no-roofline --prewarm-s 0 --no-calibration ; per-dispatch averages"
  echo "# FETCH_SIZE/WRITE_SIZE are in KB; gfx950 FETCH_SIZE under-reports wide coalesced reads by 2x (MI355X_MICROARCH.md): double it."
  python3 tools/pmc_summary.py $OUT/_pmc k_gemm k_mlp_fused k_ln k_mhsa k_outlook k_soft_ce k_bn k_adamw k_conv3x3 igemm kernel_grouped_conv; } > $OUT/${ROUND}_pmc_counters.txt
ROUND=$ROUND python3 - <<'PY'
import re, json, os, sys
sys.path.insert(0, ".")
R = os.environ["ROUND"]
txt = open(os.path.join(os.environ["OUT"], "%s_pmc_counters.txt" % R)).read()
blocks = re.split(r"\n(?=\S)", txt)
fetch = write = n = 0.0
for b in blocks:
    if b.startswith("void k_gemm_nt<") or b.startswith("void k_gemm_nt_8p<") or b.startswith("void k_gemm_nt_ws<") or b.startswith("k_gemm_nt_skinny") or b.startswith("void k_mlp_fused"):
        mf = re.search(r"FETCH_SIZE\s+avg\s+([\d.]+)\s+over (\d+)", b); mw = re.search(r"WRITE_SIZE\s+avg\s+([\d.]+)", b)
        if mf and mw:
            k = int(mf.group(2)); fetch += float(mf.group(1)) * k; write += float(mw.group(1)) * k; n += k
if n:
    per = (2.0 * fetch + write) / n * 1024.0
    import bench
    json.dump({"kernel": "k_gemm_nt_8p + k_gemm_nt_ws + k_gemm_nt + k_mlp_fused2 (all instantiations)", "hbm_bytes_per_launch": round(per), "launches": int(n),
               "formula": "(2*FETCH_SIZE + WRITE_SIZE) KB per dispatch, dispatch-weighted over the k_gemm_nt* and k_mlp_fused* instantiations",
               "source": "profiles/%s_pmc_counters.txt" % R, "src_sha256": bench.kernel_source_hash()}, open(os.path.join(os.environ["OUT"], "gemm_nt_traffic.json"), "w"))
PY
python3 tools/pmc_table.py $OUT/${ROUND}_pmc_counters.txt $OUT/${ROUND}_kernel_stats.txt > $OUT/${ROUND}_kernel_table.txt
rm -rf $OUT/_pmc
grep -A9 'k_gemm_nt_8p<1, 0>' $OUT/${ROUND}_pmc_counters.txt | head -12; cat $OUT/gemm_nt_traffic.json
