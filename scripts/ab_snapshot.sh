#!/bin/bash
# Snapshot the committed kernels (HEAD) as the A/B baseline: ab/head_csrc (sources, for
# scripts/variant_counters.py head=@ab/head_csrc) and ab/libsrbd_mpc_old.so (for scripts/ab_bench.sh),
# built by HEAD's own recipe: a tree always knows how to build itself.
set -e
cd "$(dirname "$0")/.."
rm -rf ab/head_csrc /tmp/ab_snap && mkdir -p ab/head_csrc /tmp/ab_snap
git archive HEAD biped_pympc_amd include | tar -x -C /tmp/ab_snap
cp /tmp/ab_snap/biped_pympc_amd/csrc/* ab/head_csrc/
(cd /tmp/ab_snap && python -c "from biped_pympc_amd import build; build.build()")
cp /tmp/ab_snap/biped_pympc_amd/lib/libsrbd_mpc.so ab/libsrbd_mpc_old.so
echo "A/B baseline = $(git rev-parse --short HEAD)"
