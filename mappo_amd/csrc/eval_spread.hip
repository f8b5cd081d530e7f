// eval_spread.hip — the one-launch evaluation episode on the GPU-resident simple_spread environment (see eval_spread.h): the
// actor with its weights in LDS (mlp_ep16l.h) and the environment step (mpe_core.h) in one wave per tile
#include "mlp_host.h"
#include "eval_spread.h"
