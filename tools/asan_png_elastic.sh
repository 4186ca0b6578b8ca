#!/bin/sh
# DEVELOPMENT / TEST TOOLING: build the C host layer and tools/asan_png_elastic.c under AddressSanitizer + UBSan for the CPU and run
# the program (no GPU, no Python).  Every debig_hip_* entry point the host layer refers to becomes a stub that aborts: the paths
# the program drives never reach the device.
#     sh tools/asan_png_elastic.sh [build directory, default /tmp/debig_asan_elastic]
set -e
ROOT=$(cd "$(dirname "$0")/.." && pwd)
OUT=${1:-/tmp/debig_asan_elastic}
mkdir -p "$OUT"
SAN="-fsanitize=address,undefined -fno-sanitize-recover=undefined -fno-omit-frame-pointer -g -O1"
OBJS=
for c in "$ROOT"/debigulator_amd/csrc/host/*.c; do
    o="$OUT/$(basename "$c").o"
    gcc $SAN -std=c11 -D_GNU_SOURCE -pthread -Wall -Wextra -I"$ROOT/include" -c "$c" -o "$o"
    OBJS="$OBJS $o"
done
gcc $SAN -std=c11 -D_GNU_SOURCE -Wall -Wextra -I"$ROOT/include" -c "$ROOT/tools/asan_png_elastic.c" -o "$OUT/main.o"
# the device entry points the host objects leave undefined -> aborting stubs
{
    echo '#include <stdio.h>'
    echo '#include <stdlib.h>'
    nm -u $OBJS | awk '$1 == "U" && $2 ~ /^debig_hip_/ { print $2 }' | sort -u |
        while read -r f; do printf 'long %s(void) { fputs("%s was called: the device was reached", stderr); abort(); }\n' "$f" "$f"; done
} > "$OUT/stubs.c"
gcc $SAN -c "$OUT/stubs.c" -o "$OUT/stubs.o"
gcc $SAN -pthread -o "$OUT/asan_png_elastic" "$OUT/main.o" $OBJS "$OUT/stubs.o" -lm
ASAN_OPTIONS=detect_leaks=1 "$OUT/asan_png_elastic"
