#!/bin/sh
# DEVELOPMENT / TEST TOOLING: tools/asan_png_encode_lz_emu.cpp as a stand-alone program under AddressSanitizer + UBSan, linked with the
# CPU lock-step emulator's sources (the product's kernels) compiled under the same sanitizers -- tools/simt_emu/libdebig_emu_asan.so,
# which the emulator's Makefile builds once for every test that wants it.  The program is an ordinary executable that links the
# sanitizer runtime itself: no GPU, no Python, nothing preloaded.
#     sh tools/asan_png_encode_lz_emu.sh [build directory, default /tmp/debig_asan_png_encode_lz_emu]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-/tmp/debig_asan_png_encode_lz_emu}
mkdir -p "$OUT"
make -s -C "$ROOT/tools/simt_emu" libdebig_emu_asan.so
g++ -fsanitize=address,undefined -fno-omit-frame-pointer -g -O1 -std=c++17 -Wall -o "$OUT/asan_png_encode_lz_emu" \
    "$ROOT/tools/asan_png_encode_lz_emu.cpp" -L"$ROOT/tools/simt_emu" -ldebig_emu_asan -Wl,-rpath,"$ROOT/tools/simt_emu" -lpthread
ASAN_OPTIONS=detect_leaks=1 "$OUT/asan_png_encode_lz_emu"
