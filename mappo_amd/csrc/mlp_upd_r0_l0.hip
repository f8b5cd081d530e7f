// mlp_update_kernel<RELU=false, LN=0, HEAD 0..3> — the K-chunked wide update kernel (mlp_upd.h)
#define MLP_UPD_RELU false
#define MLP_UPD_LN 0
#include "mlp_upd_launch.h"
