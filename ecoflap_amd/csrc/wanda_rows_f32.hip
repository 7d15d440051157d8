// wanda_rows_f32.hip — the f32 instances of the K7 rows-mode kernels (wanda_rows.h)
#include "wanda_rows.h"

WANDA_ROWS_UNIT(ECOFLAP_F32, f32)
