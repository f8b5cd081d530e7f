// mpe_ragged_env.h — the stepwise reset and step kernels of the MPE scenarios whose M agents have observations of different widths,
// one Discrete action each and a reward of their own (simple_adversary, simple_tag, simple_push, simple_crypto): N environments
// stepped by ONE kernel launch, one lane per environment.  Env is the scenario's traits struct, at the end of its mpe_*_core.h; the
// kernels are the same for all of them, the scenario is what Env's members forward to.
#pragma once
#include "common.h"

template <class Env>
__global__ __launch_bounds__(256) void mpe_ragged_reset_kernel(typename Env::Args a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  typename Env::State s;
  s.episode = a.episode[n] + 1;
  s.tstep = 0;
  Env::reset_env(a, n, s, s.episode);
  Env::store(a, n, s, true);
  float *o[Env::M];
#pragma unroll
  for (int m = 0; m < Env::M; ++m) o[m] = a.obs[m] + (size_t)n * Env::obs_dim(m);
  Env::write_obs(o, s);
}

template <class Env>
__global__ __launch_bounds__(256) void mpe_ragged_step_kernel(typename Env::Args a) {
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  if (n >= a.N) return;
  typename Env::State s;
  Env::load(a, n, s);
  const int stride = a.mode == 0 ? Env::U : 1;
  float reward[Env::M];
  float *o[Env::M];
#pragma unroll
  for (int m = 0; m < Env::M; ++m) o[m] = a.obs[m] + (size_t)n * Env::obs_dim(m);
  const bool done = Env::step_env(a, n, a.act + (size_t)n * Env::M * stride, stride, s, o, reward);
#pragma unroll
  for (int m = 0; m < Env::M; ++m) {
    a.rewards[(size_t)n * Env::M + m] = reward[m];
    a.dones[(size_t)n * Env::M + m] = done ? 1 : 0;
  }
  Env::store(a, n, s, done);
}

// one lane per environment, 256 to a block; who: the entry point's name in the error text
template <auto Kernel, class Args>
static int mpe_ragged_launch(const char *who, const Args &a, mappo_stream_t stream) {
  hipLaunchKernelGGL(Kernel, dim3((a.N + 255) / 256), dim3(256), 0, as_stream(stream), a);
  MAPPO_CHECK_LAUNCH(who);
  return MAPPO_OK;
}
