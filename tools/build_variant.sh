#!/bin/bash
# Build libsift_hip.so variants with extra compile flags into build_ab/<name>.so (shipped to the GPU box, git-ignored)
# usage: tools/build_variant.sh <name> "<-D flags>"
# The sources and flags are the Makefile's; only the object directory and the output differ.
set -e
R=$(cd "$(dirname "$0")/.." && pwd)
mkdir -p "$R/build_ab"
make -C "$R" -j8 lib OBJDIR="build_ab/$1.tmp" LIB="build_ab/$1.so" EXTRA="$2" ||
  { echo "variant $1: build failed"; rm -rf "$R/build_ab/$1.tmp"; exit 1; }
rm -rf "$R/build_ab/$1.tmp"
