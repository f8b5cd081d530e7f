// mlp_update_kernel<RELU=true, LN=1, HEAD 0..3> — the K-chunked wide update kernel (mlp_upd.h)
#define MLP_UPD_RELU true
#define MLP_UPD_LN 1
#include "mlp_upd_launch.h"
