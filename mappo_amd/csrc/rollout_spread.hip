// rollout_spread.hip — the one-launch rollout episode on the GPU-resident simple_spread environment (see rollout_spread.h)
#include "mlp_host.h"
#include "rollout_spread.h"
