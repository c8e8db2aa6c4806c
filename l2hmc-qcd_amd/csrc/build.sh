#!/usr/bin/env bash
# Build libl2q.so for gfx950, in-tree (see Makefile; `build.sh --clean` rebuilds from source).
set -euo pipefail
here="$(cd "$(dirname "$0")" && pwd)"
if [ "${1:-}" = "--clean" ]; then make -C "$here" clean >/dev/null; fi
# MAX_JOBS when the environment sets it, else the CPU count, at most 16: on a large shared host `nproc` counts
# CPUs this build may not use
jobs="${MAX_JOBS:-$(nproc)}"
{ [ "$jobs" -ge 1 ] && [ "$jobs" -le 16 ]; } 2>/dev/null || jobs=16
make -C "$here" -j"$jobs" all 2>&1 | grep -v "^make" || true
test -f "$here/../l2hmc/_lib/libl2q.so"
