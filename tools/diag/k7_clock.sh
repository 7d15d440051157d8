#!/bin/bash
# Builds the library with the K6 / K7 matrix-mode phase clock compiled in (its own .so, not the product's)
# -> tools/diag/_build/libecoflap_hip_k7clk.so; then on the GPU: python tools/diag/k7_clock.py
# The K6 / K7 units are compiled as one translation unit (k7_clock_unity.hip); every other object
# is the product's, by the Makefile's own list.
set -e
cd "$(dirname "$0")/../../ecoflap_amd/csrc"
UNITY="build/colsq.hip.o build/wanda.hip.o build/wanda_matrix.hip.o build/wanda_rows_f32.hip.o build/wanda_rows_f16.hip.o build/wanda_rows_bf16.hip.o"
OTHERS=""
for o in $(make -s --no-print-directory print-OBJS); do
    case " $UNITY " in *" $o "*) ;; *) OTHERS="$OTHERS $o" ;; esac
done
make -s $OTHERS
mkdir -p ../../tools/diag/_build
/opt/rocm/bin/hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -fPIC -std=c++17 -DECO_K7_CLOCK -w \
    -c ../../tools/diag/k7_clock_unity.hip -o ../../tools/diag/_build/wanda_clk.o
/opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -o ../../tools/diag/_build/libecoflap_hip_k7clk.so \
    ../../tools/diag/_build/wanda_clk.o $OTHERS
echo built tools/diag/_build/libecoflap_hip_k7clk.so
