// The K6 / K7 units as ONE translation unit, for tools/diag/k7_clock.sh (-DECO_K7_CLOCK): the phase
// clock is one __device__ array (wanda_k7.h) that K6's kernel and the K7 matrix-mode kernels stamp
// and two host entries read, and device code is not relocatable in this build — so the clock
// variant compiles the split sources together.
#include "../../ecoflap_amd/csrc/colsq.hip"
#include "../../ecoflap_amd/csrc/wanda_rows_f32.hip"
#include "../../ecoflap_amd/csrc/wanda_rows_f16.hip"
#include "../../ecoflap_amd/csrc/wanda_rows_bf16.hip"
#include "../../ecoflap_amd/csrc/wanda_matrix.hip"
#include "../../ecoflap_amd/csrc/wanda.hip"
