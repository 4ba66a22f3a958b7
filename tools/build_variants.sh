#!/bin/bash
# A/B builds of the engine library into pdmp3_amd/variants/ (git-ignored; they travel to the GPU box with gpurun).
#   bash tools/build_variants.sh name1="flags" name2="flags" ...      e.g.  base="" noslp="-fno-slp-vectorize"
# The kernels' A/B switches are -DPD_EXP_... (pdmp3_amd/csrc/decode_core.h, top): e.g. -DPD_EXP_WINDOW_SCALAR (the granule kernel's
# window sums as scalar chains), -DPD_EXP_TAPS_ROWS, -DPD_EXP_IMDCT_COPY, -DPD_EXP_SCALES_COMPUTED, -DPD_EXP_PCM_PLAIN.
# `git:<rev>` as flags builds the csrc/ of that revision instead of the working tree's.
# The sources and flags are the csrc/Makefile's (that revision's, for git:<rev>): its default library's rule with OUT and
# EXTRA set, so the list of translation units exists once.
set -e
ROOT=$(cd $(dirname $0)/.. && pwd)
mkdir -p $ROOT/pdmp3_amd/variants
for spec in "$@"; do
  name=${spec%%=*}; extra=${spec#*=}
  src=$ROOT/pdmp3_amd/csrc
  if [[ $extra == git:* ]]; then
    rev=${extra#git:}; extra=""
    src=/tmp/pdmp3_variant_$name/pdmp3_amd/csrc
    rm -rf /tmp/pdmp3_variant_$name; mkdir -p $src /tmp/pdmp3_variant_$name/include
    for f in $(git -C $ROOT ls-tree --name-only $rev pdmp3_amd/csrc/ include/); do git -C $ROOT show $rev:$f > /tmp/pdmp3_variant_$name/$f; done
  fi
  out=$ROOT/pdmp3_amd/variants/$name.so
  make -B -C $src OUT=$out EXTRA="$extra -Wno-pass-failed" $out &
done
wait
ls -la $ROOT/pdmp3_amd/variants/
