// mpe_world_comm_core.h — the MPE `simple_world_comm` environment as device functions: reset, action decoding, one environment step
// and the observation write, one lane per environment.  Shared by every launch that steps this environment, so a step computes the
// same float64 values whichever launch runs it.  Reference sites: see mpe_world_comm_env.hip.
//
// Fixed shape (num_adversaries = 4, num_good_agents = 2, num_landmarks = 1; 2 food items and 2 forests are constants of the scenario):
// agents 0..3 are the ADVERSARIES (size 0.075, accel 3, max_speed 1), agent 0 their LEADER, agents 4, 5 the GOOD agents (size 0.045,
// accel 4, max_speed 1.3).  The landmarks in world order: [landmark (0.2), food0, food1 (0.03), forest0, forest1 (0.3)]; only landmark
// 0 collides.  Every agent moves, Discrete(5); the leader also says one of dim_c = 4 words — MultiDiscrete([[0, 4], [0, 3]]) — and
// the word of THIS step stands in every adversary's observation.  Observation of agent m: own velocity, own position, the five
// landmarks relative to it, the five other agents relative to it in world order, then
//   adversaries (34): the velocities of the two good agents, own in_forest flags (+-1 per forest), the leader's word (4)
//   good agents (28): own in_forest flags, the velocity of the other good agent.
// An other agent's position — and a good one's velocity — is ZERO unless it is visible: both in the same forest, or both in no
// forest, or the observer is the leader.  The world is NOT collaborative: each agent receives its own reward.
//
// The action force is accel * (accel * u), as in simple_tag (mpe_tag_core.h): 9 per unit of u for an adversary, 16 for a good agent.
//
// Reset draws: Philox stream (seed, episode), mpe_uniform index MPE_WC_DRAWS * n + k for environment n —
//   k = 2 a, 2 a + 1            position of agent a, U(-1,1)                          (k = 0 .. 11)
//   k = 12 + 2 l, 13 + 2 l      position of landmark l, 0.8 U(-1,1)                   (k = 12 .. 21)
//   k = 22 .. 31                unused
// so no two draws of one (seed, episode) share an index.
#pragma once
#include "mpe_tag_core.h"                                           // mpe_tag_contact: the soft-collision force of core.py:289-322

#define MPE_WC_M 6
#define MPE_WC_ADV 4                                                // agents 0 .. 3 are adversaries, 0 the leader; 4, 5 are good
#define MPE_WC_L 5                                                  // landmark, food0, food1, forest0, forest1
#define MPE_WC_FOOD 1                                               // first food landmark
#define MPE_WC_FOREST 3                                             // first forest landmark
#define MPE_WC_U 5                                                  // width of a move one-hot (mode 0)
#define MPE_WC_C 4                                                  // dim_c: width of the leader's word
#define MPE_WC_ACT_LEADER (MPE_WC_U + MPE_WC_C)                     // mode 0: the leader's two one-hots side by side
#define MPE_WC_ACT_IDX (MPE_WC_M + 1)                               // mode 1: leader move, leader word, agents 1 .. 5
#define MPE_WC_OBS_A 34                                             // adversary: 4 + 2 L + 2 (M - 1) + 4 + 2 + 4
#define MPE_WC_OBS_G 28                                             // good agent: 4 + 2 L + 2 (M - 1) + 2 + 2
#define MPE_WC_SHARE (MPE_WC_ADV * MPE_WC_OBS_A + 2 * MPE_WC_OBS_G) // the six observations side by side: 192
#define MPE_WC_DRAWS 32

__host__ __device__ constexpr int mpe_wc_obs_dim(int m) { return m < MPE_WC_ADV ? MPE_WC_OBS_A : MPE_WC_OBS_G; }
// where agent m's observation starts in the centralized share row (the six observations side by side)
__host__ __device__ constexpr int mpe_wc_obs_off(int m) { return m < MPE_WC_ADV ? m * MPE_WC_OBS_A : MPE_WC_ADV * MPE_WC_OBS_A + (m - MPE_WC_ADV) * MPE_WC_OBS_G; }
// per-agent physics (simple_world_comm.py:25-28) and the landmarks' sizes (:35,42,49)
__host__ __device__ constexpr double mpe_wc_size(int m) { return m < MPE_WC_ADV ? 0.075 : 0.045; }
__host__ __device__ constexpr double mpe_wc_accel(int m) { return m < MPE_WC_ADV ? 3.0 : 4.0; }
__host__ __device__ constexpr double mpe_wc_max_speed(int m) { return m < MPE_WC_ADV ? 1.0 : 1.3; }
#define MPE_WC_LSIZE 0.2
#define MPE_WC_FOOD_SIZE 0.03
#define MPE_WC_FOREST_SIZE 0.3

struct MpeWcArgs {
  double *apos, *avel, *lpos;      // agents [N][6][2], [N][6][2]; landmarks [N][5][2]
  int32_t *tstep;                  // [N] steps since the last reset
  int64_t *episode;                // [N] resets so far (Philox counter)
  const float *act[MPE_WC_M];      // mode 0: one-hots / probabilities, [N][9] of the leader and [N][5] x 5 | mode 1: act[0] = indices [N][7]
  float *obs[MPE_WC_M];            // [N][34] x 4, [N][28] x 2
  float *rewards;                  // [N][6]: one per agent
  uint8_t *dones;                  // [N][6] bool bytes
  int N, T, mode;
  uint64_t seed;
};

// the state one lane holds
struct MpeWcState {
  double p[MPE_WC_M][2], v[MPE_WC_M][2], lp[MPE_WC_L][2];
  int32_t tstep;
  int64_t episode;
};

// what the six actions of one environment decode to: u = (a1 - a2, a3 - a4) per agent, and the leader's word as it enters the
// observations (mode 0: the four floats of its second head; mode 1: the one-hot of its index)
struct MpeWcAction {
  double u[MPE_WC_M][2];
  float c[MPE_WC_C];
};

// mode 1, one index as fp32 -> what it decodes to (shared with the one-launch episode, rollout_world_comm.h, which reads the indices
// from its LDS action tile): a move index, clamped to 0 .. 4, is u = (a1 - a2, a3 - a4) of its one-hot; a word index, clamped to
// 0 .. 3, is its one-hot
__device__ __forceinline__ void mpe_wc_move_idx(float idx, double (&u)[2]) {
  int k = (int)idx;
  k = k < 0 ? 0 : (k > 4 ? 4 : k);
  u[0] = k == 1 ? 1.0 : (k == 2 ? -1.0 : 0.0);
  u[1] = k == 3 ? 1.0 : (k == 4 ? -1.0 : 0.0);
}
__device__ __forceinline__ void mpe_wc_word_idx(float idx, float (&c)[MPE_WC_C]) {
  int w = (int)idx;
  w = w < 0 ? 0 : (w > MPE_WC_C - 1 ? MPE_WC_C - 1 : w);
#pragma unroll
  for (int j = 0; j < MPE_WC_C; ++j) c[j] = j == w ? 1.f : 0.f;
}

// environment.py:194-256 for environment n.  The MultiDiscrete split (:198-205) cuts the leader's [9] into move [0, 5) and word
// [5, 9); indices out of range go to the nearest.
__device__ __forceinline__ void mpe_wc_decode(const MpeWcArgs &a, int n, MpeWcAction &d) {
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m) {
    if (a.mode == 0) {
      const float *am = a.act[m] + (size_t)n * (m == 0 ? MPE_WC_ACT_LEADER : MPE_WC_U);
      d.u[m][0] = (double)am[1] - (double)am[2]; d.u[m][1] = (double)am[3] - (double)am[4];
    } else {
      mpe_wc_move_idx(a.act[0][(size_t)n * MPE_WC_ACT_IDX + (m == 0 ? 0 : m + 1)], d.u[m]);
    }
  }
  if (a.mode == 0) {
#pragma unroll
    for (int j = 0; j < MPE_WC_C; ++j) d.c[j] = a.act[0][(size_t)n * MPE_WC_ACT_LEADER + MPE_WC_U + j];
  } else {
    mpe_wc_word_idx(a.act[0][(size_t)n * MPE_WC_ACT_IDX + 1], d.c);
  }
}

// scenario.reset_world (simple_world_comm.py:100-112): agents U(-1,1)^2 at rest, all five landmarks 0.8 U(-1,1)^2
__device__ __forceinline__ void mpe_wc_reset_env(const MpeWcArgs &a, int n, MpeWcState &s, int64_t ep) {
#pragma clang fp contract(off)   // as in mpe_wc_step_env, which inlines this
  const uint64_t base = (uint64_t)n * MPE_WC_DRAWS;
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m) {
    s.p[m][0] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m);
    s.p[m][1] = mpe_uniform(a.seed, (uint64_t)ep, base + 2 * m + 1);
    s.v[m][0] = s.v[m][1] = 0.0;
  }
#pragma unroll
  for (int l = 0; l < MPE_WC_L; ++l) {
    s.lp[l][0] = 0.8 * mpe_uniform(a.seed, (uint64_t)ep, base + 2 * MPE_WC_M + 2 * l);
    s.lp[l][1] = 0.8 * mpe_uniform(a.seed, (uint64_t)ep, base + 2 * MPE_WC_M + 2 * l + 1);
  }
}

// scenario.is_collision (simple_world_comm.py:125-129) from delta = p_first - p_second
__device__ __forceinline__ bool mpe_wc_touch(double dx, double dy, double dist_min) {
#pragma clang fp contract(off)
  return sqrt(dx * dx + dy * dy) < dist_min;
}

__device__ __forceinline__ double mpe_wc_dist(double dx, double dy) {
#pragma clang fp contract(off)
  return sqrt(dx * dx + dy * dy);
}

// scenario.observation (simple_world_comm.py:225-288) of every agent; c: the leader's word (state.c of agent 0), zeros after a reset
__device__ __forceinline__ void mpe_wc_write_obs(float *const (&obs)[MPE_WC_M], const MpeWcState &s, const float (&c)[MPE_WC_C]) {
#pragma clang fp contract(off)
  bool in[MPE_WC_M][2];                                             // agent m inside forest f
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m)
#pragma unroll
    for (int f = 0; f < 2; ++f)
      in[m][f] = mpe_wc_touch(s.p[m][0] - s.lp[MPE_WC_FOREST + f][0], s.p[m][1] - s.lp[MPE_WC_FOREST + f][1],
                              mpe_wc_size(m) + MPE_WC_FOREST_SIZE);
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m) {
    float *o = obs[m];
    int k = 0;
    o[k++] = (float)s.v[m][0]; o[k++] = (float)s.v[m][1];
    o[k++] = (float)s.p[m][0]; o[k++] = (float)s.p[m][1];
#pragma unroll
    for (int l = 0; l < MPE_WC_L; ++l) { o[k++] = (float)(s.lp[l][0] - s.p[m][0]); o[k++] = (float)(s.lp[l][1] - s.p[m][1]); }
    bool vis[MPE_WC_M];
#pragma unroll
    for (int i = 0; i < MPE_WC_M; ++i)                              // :255; the leader sees everybody
      vis[i] = (in[m][0] && in[i][0]) || (in[m][1] && in[i][1]) || (!in[m][0] && !in[i][0] && !in[m][1] && !in[i][1]) || m == 0;
#pragma unroll
    for (int i = 0; i < MPE_WC_M; ++i)
      if (i != m) {
        o[k++] = vis[i] ? (float)(s.p[i][0] - s.p[m][0]) : 0.f;
        o[k++] = vis[i] ? (float)(s.p[i][1] - s.p[m][1]) : 0.f;
      }
    if (m >= MPE_WC_ADV) { o[k++] = in[m][0] ? 1.f : -1.f; o[k++] = in[m][1] ? 1.f : -1.f; }      // good agents: in_forest before other_vel
#pragma unroll
    for (int i = MPE_WC_ADV; i < MPE_WC_M; ++i)
      if (i != m) { o[k++] = vis[i] ? (float)s.v[i][0] : 0.f; o[k++] = vis[i] ? (float)s.v[i][1] : 0.f; }
    if (m < MPE_WC_ADV) {
      o[k++] = in[m][0] ? 1.f : -1.f; o[k++] = in[m][1] ? 1.f : -1.f;
#pragma unroll
      for (int j = 0; j < MPE_WC_C; ++j) o[k++] = c[j];
    }
  }
}

__device__ __forceinline__ void mpe_wc_load(const MpeWcArgs &a, int n, MpeWcState &s) {
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      s.p[m][d] = a.apos[((size_t)n * MPE_WC_M + m) * 2 + d];
      s.v[m][d] = a.avel[((size_t)n * MPE_WC_M + m) * 2 + d];
    }
#pragma unroll
  for (int l = 0; l < MPE_WC_L; ++l) { s.lp[l][0] = a.lpos[((size_t)n * MPE_WC_L + l) * 2]; s.lp[l][1] = a.lpos[((size_t)n * MPE_WC_L + l) * 2 + 1]; }
  s.tstep = a.tstep[n];
  s.episode = a.episode[n];
}

// landmarks: also the landmark positions and the episode counter (they change only at a reset)
__device__ __forceinline__ void mpe_wc_store(const MpeWcArgs &a, int n, const MpeWcState &s, bool landmarks) {
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m)
#pragma unroll
    for (int d = 0; d < 2; ++d) {
      a.apos[((size_t)n * MPE_WC_M + m) * 2 + d] = s.p[m][d];
      a.avel[((size_t)n * MPE_WC_M + m) * 2 + d] = s.v[m][d];
    }
  a.tstep[n] = s.tstep;
  if (landmarks) {
#pragma unroll
    for (int l = 0; l < MPE_WC_L; ++l) { a.lpos[((size_t)n * MPE_WC_L + l) * 2] = s.lp[l][0]; a.lpos[((size_t)n * MPE_WC_L + l) * 2 + 1] = s.lp[l][1]; }
    a.episode[n] = s.episode;
  }
}

// One step of environment n on the state the lane holds: the decoded actions -> forces, collision forces, integration with the speed
// clamp, per-agent rewards, time-limit done, reset-on-done, observations (obs[m]: the environment's own row of agent m, 34 or 28
// floats).  reward[m]: what agent m receives.  Returns done (the state is then the reset state, and the word in the observations
// is zero).
__device__ __forceinline__ bool mpe_wc_step_env(const MpeWcArgs &a, int n, const MpeWcAction &act, MpeWcState &s, float *const (&obs)[MPE_WC_M],
                                                float (&reward)[MPE_WC_M]) {
  // contraction pinned off for the reason given in mpe_step_env: the body may be inlined into more than one kernel, and they must
  // agree to the bit
#pragma clang fp contract(off)
  double f[MPE_WC_M][2];
  // ---- action -> force (environment.py:235-238: u *= accel; core.py:229-238: force = (mass * accel) * u, mass 1, no noise) ----
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m) {
    const double acc = mpe_wc_accel(m);
    f[m][0] = acc * (act.u[m][0] * acc); f[m][1] = acc * (act.u[m][1] * acc);
  }
  // ---- soft-collision forces (core.py:241-263,289-322): entity pairs a < b in world order, agents 0 .. 5 then landmark 0 as entity
  // 6 (food and forests do not collide); f_a is added to the force on a, then f_b to the force on b.  The 21 pairs are walked by a
  // ROLLED loop over the uniform (a, b), entities and forces picked by selects, as in mpe_tag_step_env: same operations in the same
  // order as unrolled, without the registers of 21 float64 exp / log1p side by side ----
  {
    int pa = 0, pb = 1;
#pragma nounroll
    for (int pair = 0; pair < 21; ++pair) {
      double ax = s.p[0][0], ay = s.p[0][1], bx = s.lp[0][0], by = s.lp[0][1];
#pragma unroll
      for (int m = 1; m < MPE_WC_M; ++m) { ax = pa == m ? s.p[m][0] : ax; ay = pa == m ? s.p[m][1] : ay; }
#pragma unroll
      for (int m = 1; m < MPE_WC_M; ++m) { bx = pb == m ? s.p[m][0] : bx; by = pb == m ? s.p[m][1] : by; }
      const double sa = pa < MPE_WC_ADV ? mpe_wc_size(0) : mpe_wc_size(MPE_WC_ADV);
      const double sb = pb < MPE_WC_ADV ? mpe_wc_size(0) : (pb < MPE_WC_M ? mpe_wc_size(MPE_WC_ADV) : MPE_WC_LSIZE);
      double fx, fy;
      mpe_tag_contact(ax - bx, ay - by, sa + sb, fx, fy);
#pragma unroll
      for (int m = 0; m < MPE_WC_M; ++m) {
        const double gx = pa == m ? fx : -fx, gy = pa == m ? fy : -fy;     // f_a = force, f_b = -force
        const bool hit = pa == m || pb == m;
        f[m][0] = hit ? gx + f[m][0] : f[m][0]; f[m][1] = hit ? gy + f[m][1] : f[m][1];
      }
      if (++pb == MPE_WC_M + 1) { ++pa; pb = pa + 1; }
    }
  }
  // ---- integrate (core.py:265-278: damping 0.25, the max_speed clamp, dt 0.1) ----
#pragma unroll
  for (int m = 0; m < MPE_WC_M; ++m) {
    double vx = s.v[m][0] * (1.0 - 0.25), vy = s.v[m][1] * (1.0 - 0.25);
    vx += f[m][0] * 0.1; vy += f[m][1] * 0.1;
    const double speed = sqrt(vx * vx + vy * vy);
    if (speed > mpe_wc_max_speed(m)) { vx = vx / speed * mpe_wc_max_speed(m); vy = vy / speed * mpe_wc_max_speed(m); }
    s.v[m][0] = vx; s.v[m][1] = vy;
    s.p[m][0] += vx * 0.1; s.p[m][1] += vy * 0.1;
  }
  // ---- rewards (simple_world_comm.py:141-199; world.collaborative is not set: each agent keeps its own, environment.py:49-50,142) ----
  // adversary (shape = True): -0.1 * distance to the nearest good agent, then +5 per (good agent, adversary) pair in contact —
  // every adversary's pairs, not only its own
#pragma unroll
  for (int m = 0; m < MPE_WC_ADV; ++m) {
    double dmin = mpe_wc_dist(s.p[MPE_WC_ADV][0] - s.p[m][0], s.p[MPE_WC_ADV][1] - s.p[m][1]);
    const double d1 = mpe_wc_dist(s.p[MPE_WC_ADV + 1][0] - s.p[m][0], s.p[MPE_WC_ADV + 1][1] - s.p[m][1]);
    dmin = d1 < dmin ? d1 : dmin;
    double r = 0.0 - 0.1 * dmin;
#pragma unroll
    for (int g = MPE_WC_ADV; g < MPE_WC_M; ++g)
#pragma unroll
      for (int v = 0; v < MPE_WC_ADV; ++v)
        if (mpe_wc_touch(s.p[g][0] - s.p[v][0], s.p[g][1] - s.p[v][1], mpe_wc_size(g) + mpe_wc_size(v))) r += 5.0;
    reward[m] = (float)r;
  }
  // good agent (shape = False): -5 per adversary touching it, -2 bound(|x|) - 2 bound(|y|), +2 per food item touched, +0.05 *
  // distance to the nearest food item
#pragma unroll
  for (int g = MPE_WC_ADV; g < MPE_WC_M; ++g) {
    double r = 0.0;
#pragma unroll
    for (int v = 0; v < MPE_WC_ADV; ++v)
      if (mpe_wc_touch(s.p[v][0] - s.p[g][0], s.p[v][1] - s.p[g][1], mpe_wc_size(v) + mpe_wc_size(g))) r -= 5.0;
    r -= 2.0 * mpe_tag_bound(fabs(s.p[g][0]));
    r -= 2.0 * mpe_tag_bound(fabs(s.p[g][1]));
    double fmin_ = 0.0;
#pragma unroll
    for (int l = 0; l < 2; ++l) {
      const double dx = s.p[g][0] - s.lp[MPE_WC_FOOD + l][0], dy = s.p[g][1] - s.lp[MPE_WC_FOOD + l][1];
      if (mpe_wc_touch(dx, dy, mpe_wc_size(g) + MPE_WC_FOOD_SIZE)) r += 2.0;
      const double d = mpe_wc_dist(-dx, -dy);                        // food - agent, as the reference writes it
      fmin_ = (l == 0 || d < fmin_) ? d : fmin_;
    }
    r += 0.05 * fmin_;
    reward[g] = (float)r;
  }
  const int t = s.tstep + 1;
  const bool done = t >= a.T;                                       // environment.py:179-185
  float c[MPE_WC_C];
#pragma unroll
  for (int j = 0; j < MPE_WC_C; ++j) c[j] = done ? 0.f : act.c[j];  // reset_world zeroes state.c
  if (done) {                                                       // vec-env wrappers: the returned obs are the reset obs
    s.episode += 1;
    mpe_wc_reset_env(a, n, s, s.episode);
    s.tstep = 0;
  } else {
    s.tstep = t;
  }
  mpe_wc_write_obs(obs, s, c);
  return done;
}
