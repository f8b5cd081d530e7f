// rollout_spread.hip — the one-launch rollout episode on the GPU-resident simple_spread environment (see rollout_spread.h)
#define MLP_TU_SPREAD
#include "mlp_impl.h"
