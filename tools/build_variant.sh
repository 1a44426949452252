#!/bin/bash
# Builds an EXPERIMENT variant of libsfgs.so into skyfall-gs_amd/sfgs/_exp/lib_<name>.so (git-ignored; travels to the GPU box;
# compare with tools/ab.sh). The shipped sources carry no experiment knobs: a variant is the sources + patches + flags,
# built by csrc/Makefile (its source list, its per-file flags) in a scratch copy of skyfall-gs_amd/csrc.
# usage: tools/build_variant.sh <name> "<flags>" [patch ...]        (patches: tools/variants/*.patch, applied with -p1
#        from the repo root, in order; "" for no flags)
#   tools/build_variant.sh nop1 "-DSFGS_BWD_ABLATE=2" tools/variants/bwd_lab_r5.patch
#   FLAG_FILES=ssim.hip tools/build_variant.sh ssim_ilp "-mllvm -amdgpu-sched-strategy=max-ilp"
# FLAG_FILES="a.hip b.hip" (environment): the flags go to these files only (default: the Makefile's FLAG_FILES).
set -e
name=$1; flags=${2:-}; shift; [ $# -gt 0 ] && shift
ROOT="$(cd "$(dirname "$0")/.." && pwd)"
SRC=$ROOT/skyfall-gs_amd/csrc
W=$SRC/_obj/var_$name
rm -rf "$W"; mkdir -p "$W/skyfall-gs_amd/csrc" "$W/include" "$ROOT/skyfall-gs_amd/sfgs/_exp"
cp "$SRC"/Makefile "$SRC"/*.hip "$SRC"/*.cpp "$SRC"/*.h "$W/skyfall-gs_amd/csrc/"; cp "$ROOT"/include/*.h "$W/include/"
for p in "$@"; do ( cd "$W" && patch -s -p1 < "$ROOT/$p" ); done
make -C "$W/skyfall-gs_amd/csrc" -j8 OUT="$ROOT/skyfall-gs_amd/sfgs/_exp/lib_$name.so" VARIANT_FLAGS="$flags" \
     ${FLAG_FILES:+FLAG_FILES="$FLAG_FILES"}
echo built skyfall-gs_amd/sfgs/_exp/lib_$name.so
