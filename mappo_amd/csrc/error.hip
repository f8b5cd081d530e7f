// error.hip — last-error text and ABI version of libmappo_hip.so.
#include "common.h"
#include <string.h>

static thread_local char g_err[512] = "";

void mappo_set_error(const char *fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
}

extern "C" const char *mappo_last_error(void) { return g_err; }
extern "C" int mappo_abi_version(void) { return 14; }   // 14: mappo_actor_critic_update_group / mappo_reduce_clip_adam_group (the agents' updates of a separated run in one launch); 4: the MultiDiscrete entry points (mappo_*_md); 5: simple_reference (mappo_mpe_reference_*, mappo_rollout_episode_reference); 6: simple_speaker_listener (mappo_mpe_comm_*, mappo_rollout_episode_comm); 7: simple_adversary (mappo_mpe_adversary_*, mappo_rollout_episode_adversary); 8: mappo_train_prologue / mappo_train_epilogue; 9: simple_tag (mappo_mpe_tag_*, mappo_rollout_episode_tag); 10: simple_push (mappo_mpe_push_*, mappo_rollout_episode_push); 11: simple_crypto (mappo_mpe_crypto_*, mappo_rollout_episode_crypto); 12: simple_world_comm (mappo_mpe_world_comm_*); 13: MAPPO_MAX_IN_DIM 2048 (in_dim 513..2048 on the Discrete path)

ProfSlot g_prof[MAPPO_PROF_COUNT] = {};

extern "C" int mappo_profile_arm(int32_t kernel_id, void *ev_start, void *ev_stop) {
  MAPPO_REQUIRE(kernel_id >= 0 && kernel_id < MAPPO_PROF_COUNT, "profile_arm: kernel_id %d", kernel_id);
  g_prof[kernel_id].start = (hipEvent_t)ev_start;
  g_prof[kernel_id].stop = (hipEvent_t)ev_stop;
  return MAPPO_OK;
}
