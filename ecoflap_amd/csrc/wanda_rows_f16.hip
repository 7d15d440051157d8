// wanda_rows_f16.hip — the f16 instances of the K7 rows-mode kernels (wanda_rows.h)
#include "wanda_rows.h"

WANDA_ROWS_UNIT(ECOFLAP_F16, f16)
