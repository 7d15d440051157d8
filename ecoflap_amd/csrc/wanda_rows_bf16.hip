// wanda_rows_bf16.hip — the bf16 instances of the K7 rows-mode kernels (wanda_rows.h)
#include "wanda_rows.h"

WANDA_ROWS_UNIT(ECOFLAP_BF16, bf16)
