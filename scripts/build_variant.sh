#!/bin/bash
# scripts/build_variant.sh <name> [UNIT=<file stem>] [extra hipcc flags...]  -> scripts/ubench/lib_<name>.so   (kernel A/B builds)
# only ONE unit is recompiled with the flags: rome_conv_pose2 (the Pose2 / bearing-range sweep) unless the first argument after the name
# is of the form UNIT=<file stem> (UNIT=rome_conv_pose3, UNIT=rome_kde, ...); the other units come from rome.jl_amd/build
# (python rome.jl_amd/_build.py first).  Run with ROME_MI355_LIB=scripts/ubench/lib_<name>.so
R=$(cd "$(dirname "$0")/.." && pwd); n=$1; shift
u=rome_conv_pose2
case "$1" in UNIT=*) u=${1#UNIT=}; shift;; esac
rm -f $R/scripts/ubench/lib_$n.so
hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -Wno-pass-failed "$@" -c $R/rome.jl_amd/csrc/$u.hip -o /tmp/variant_$n.o 2>&1 | grep -E "error" | head
hipcc --offload-arch=gfx950 -shared -fPIC -o $R/scripts/ubench/lib_$n.so /tmp/variant_$n.o $(for f in $R/rome.jl_amd/csrc/*.hip; do b=$(basename $f .hip); [ $b = $u ] || echo $R/rome.jl_amd/build/$b.o; done)
test -f $R/scripts/ubench/lib_$n.so
