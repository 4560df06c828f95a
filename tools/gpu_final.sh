#!/bin/bash
# End-of-round check on a fresh box: build stamp, smoke(), the GPU test-suite, the bench line with every leg (--full).
cd $GRAFT_REPO_ROOT
OUT=${OUT:-bench_out/final}; mkdir -p "$OUT"
python -c "import __graft_entry__ as g; g.smoke(); print('SMOKE_OK')" 2>&1 | grep -v amdgpu | tail -3
timeout 1500 python -m pytest tests -m gpu -x -q > "$OUT/tests.txt" 2>&1; grep -n "passed\|failed\|rror" "$OUT/tests.txt" | head -5
timeout 900 python bench.py --full 2>"$OUT/bench_err.txt" | tail -1 > "$OUT/bench_line.json"; python -c "
import json; r=json.load(open('$OUT/bench_line.json')); print('bench', round(r['value']), r['ms_per_step'], r['roofline']['frac'], r['grad_inf_err_vs_cpu']['f32']['grad_inf_err_max'], r['cpu_baseline']['value'], r['cpu_baseline'].get('sparse_lu_flops'))"
