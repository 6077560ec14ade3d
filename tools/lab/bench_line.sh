#!/bin/bash
# one summary line of a full bench run (roofline, forward-only and secondary lines included): tools/lab/bench_line.sh [bench.py flags]
out=$(mktemp) && python bench.py --full "$@" 2>/dev/null | tail -1 > "$out" && python tools/lab/show_bench.py "$out"; rc=$?; rm -f "$out"; exit $rc
