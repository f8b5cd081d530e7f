// mlp_update16_md_kernel / mlp_update16_md_dual_kernel<RELU=true, LN=0> — the MultiDiscrete actor on 16-sample tiles (mlp_upd16.h)
#define MLP_UPD_RELU true
#define MLP_UPD_LN 0
#define MLP_UPD_MD
#include "mlp_upd16_launch.h"
