// rollout_spread.hip — the one-launch rollout episodes on the GPU-resident environments: simple_spread (see rollout_spread.h) and
// simple_reference (see rollout_reference.h) and, for the separated runner, simple_speaker_listener (see rollout_comm.h),
// simple_adversary and simple_crypto (see rollout_sep_img.h), simple_tag (see rollout_tag.h), simple_push (see rollout_push.h) and
// simple_world_comm (see rollout_world_comm.h: the actors and the environments, the critics run afterwards)
#include "mlp_host.h"
#include "rollout_spread.h"
#include "rollout_reference.h"
#include "rollout_comm.h"
#include "rollout_sep_img.h"
#include "rollout_tag.h"
#include "rollout_push.h"
#include "rollout_world_comm.h"
