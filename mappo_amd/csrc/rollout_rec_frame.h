// rollout_rec_frame.h — what the one-launch RECURRENT rollout episodes share (rollout_spread_rec.h, rollout_smac_rec.h): a workgroup
// of eight waves owns one 16-row tile of whole environments and walks all T steps alone, waves 0..3 the actor and 4..7 the critic,
// each group through gru_step3_tiles (Step3Src::Episode) with its trunk staged once into LDS.  An episode's LDS map (Ld below)
// names the offsets imgA / imgC (trunk images), hsA / hsC (state tiles [2][16][REC_HS]), mk and act ([16] each).
#pragma once
#include "gru_step3.h"
#include "mlp_ep16l.h"

#define REC_HS 68                                                   // row stride of the LDS state tiles (rows 4 banks apart)
#define REC_WAVES 8
#define REC_LDS_MAX (LDS_DYN_MAX - (int)(2 * sizeof(Step3Shared)))  // dynamic LDS beside the two networks' exchange buffers

// The fields of gru_step3_tiles' `ep` that every episode has; an episode's own type adds HEAD_BLOCKS, avail, late() and fill().
template <int LN>
struct Step3EpFrame {
  Trunk16L<LN> tw;                 // this lane's view of its network's trunk image
  const float *xrow;               // this lane's input row (LDS)
  const float *hs;                 // [16][hs_stride] previous states of the tile
  float *hs_next;                  // ... of the next step
  const float *mk;                 // [16] masks of the step
  float *act;                      // [16] sampled actions of the tile rows
  int hs_stride, row0, R;          // first buffer row of the tile, rows that exist
  int64_t so;                      // t * B
  uint64_t ctr;                    // sampling counter of the step
};

// ---- kernel prologue, every thread: both trunks, the tile's states and masks of slot 0 -> LDS (the input tiles: each kernel) ----
template <int LN, class Ld>
__device__ __forceinline__ void rec_stage(float *lds, const GruFwdArgs &a, const GruFwdArgs &c, const float *rnn_a, const float *rnn_c,
                                          const float *mask_buf, const int i0, const int Rv) {
  const int tid = threadIdx.x, nt = REC_WAVES * WAVE;
  epl_stage<LN, 0>(lds + Ld::imgA, a.params, a.off, a.desc);
  epl_stage<LN, 0>(lds + Ld::imgC, c.params, c.off, c.desc);
  for (int k = tid; k < 16 * HID; k += nt) {
    const int row = k >> 6, u = k & 63;
    lds[Ld::hsA + row * REC_HS + u] = row < Rv ? rnn_a[(int64_t)(i0 + row) * HID + u] : 0.f;
    lds[Ld::hsC + row * REC_HS + u] = row < Rv ? rnn_c[(int64_t)(i0 + row) * HID + u] : 0.f;
  }
  if (tid < 16) { lds[Ld::mk + tid] = tid < Rv ? mask_buf[i0 + tid] : 0.f; lds[Ld::act + tid] = 0.f; }
}

// ---- one network's four waves (HM 2: the actor, 1: the critic): what a role knows before its first step ----
struct RecRole {
  int lane, n, q, i0, Rv, jr;      // i0: first buffer row of the tile, Rv: rows that exist (the last tile may be partial), jr: n or 0
  bool ok;                         // n < Rv
  float *mk, *act, *hs;            // LDS: masks, actions, this network's two state tiles
  uint64_t ctr0;                   // sampling counter of step 0
};
template <int HM, class Ld, int LN, class EP>
__device__ __forceinline__ RecRole rec_role_begin(const GruFwdArgs &p, float *lds, const int64_t B, const int G, const int M, const int w,
                                                  Step3W<LN> &W, EP &ep) {
  RecRole r;
  r.lane = threadIdx.x & (WAVE - 1); r.n = r.lane & 15; r.q = r.lane >> 4;
  r.i0 = (int)blockIdx.x * G * M;
  r.Rv = (int)(B - r.i0 < G * M ? B - r.i0 : G * M);
  r.ok = r.n < r.Rv;
  r.jr = r.ok ? r.n : 0;
  r.mk = lds + Ld::mk; r.act = lds + Ld::act;
  r.hs = lds + (HM == 2 ? Ld::hsA : Ld::hsC);
  const float *img = lds + (HM == 2 ? Ld::imgA : Ld::imgC);
  gru_step3_load<Step3Src::Episode, LN>(W, p, w, r.n, r.q);        // GRU slices, biases, head rows: registers (the trunk: LDS)
  r.ctr0 = p.counter + (p.counter_dev ? *p.counter_dev : 0ull);     // read once: the word is fixed for the launch
  ep.tw.m = img + r.n * EPL_WS + 4 * r.q; ep.tw.v = img + 4 * r.q;
  ep.mk = r.mk; ep.act = r.act; ep.hs_stride = REC_HS; ep.row0 = r.i0; ep.R = r.Rv;
  return r;
}

// step t reads state half t & 1 and writes the new state (before the mask) into the other half
template <class EP>
__device__ __forceinline__ void rec_step_begin(EP &ep, const RecRole &r, const int t, const int64_t so) {
  ep.hs = r.hs + (t & 1) * 16 * REC_HS;
  ep.hs_next = r.hs + ((t + 1) & 1) * 16 * REC_HS;
  ep.so = so; ep.ctr = r.ctr0 + (uint64_t)t;
}
// the new state x (1 - dones_env) -> rows row0 .. of slot t + 1, behind the barrier that publishes the masks (sl: the lane, as the caller shows it to the compiler)
__device__ __forceinline__ void rec_store_state(float *rnn, const g4_t &h, const RecRole &r, const int sl, const int64_t row0, const int w) {
  const int sn = sl & 15, sq = sl >> 4;
  if (sn < r.Rv) {
    const float keep = r.mk[sn];
    g4u_t o; o[0] = h[0] * keep; o[1] = h[1] * keep; o[2] = h[2] * keep; o[3] = h[3] * keep;
    *reinterpret_cast<g4u_t *>(rnn + (row0 + sn) * HID + 16 * w + 4 * sq) = o;
  }
}

// ---- host ---------------------------------------------------------------------------------------------
static int rec_episode_check(const mappo_net_desc *actor_desc, const mappo_net_desc *critic_desc, int32_t N, int32_t M, const char *who) {
  MAPPO_REQUIRE(actor_desc && critic_desc, "%s: bad arguments (null pointer)", who);
  MAPPO_REQUIRE(actor_desc->recurrent && critic_desc->recurrent, "%s: needs recurrent network descriptors (actor and critic)", who);
  if (int rc = check_desc_common(actor_desc, who)) return rc;      // (actor out_dim <= MAPPO_MAX_ACTIONS among them)
  if (int rc = check_desc_common(critic_desc, who)) return rc;
  MAPPO_REQUIRE(actor_desc->in_dim <= MAXD && critic_desc->in_dim <= MAXD, "%s: in_dim %d / %d: both networks must be narrow (<= %d); wider "
                "inputs step one launch at a time", who, actor_desc->in_dim, critic_desc->in_dim, MAXD);
  MAPPO_REQUIRE(actor_desc->layer_N <= 1 && critic_desc->layer_N <= 1, "%s: layer_N %d / %d: at most one hidden layer (layer_N <= 1)", who,
                actor_desc->layer_N, critic_desc->layer_N);
  MAPPO_REQUIRE(actor_desc->layer_N == critic_desc->layer_N && actor_desc->use_relu == critic_desc->use_relu,
                "%s: actor and critic must share layer_N and the activation", who);
  MAPPO_REQUIRE(critic_desc->out_dim == 1, "%s: critic out_dim must be 1", who);
  MAPPO_REQUIRE((int64_t)N * M <= INT32_MAX / MAXD, "%s: N*M = %lld rows exceed the int32 row indices", who, (long long)N * M);
  return MAPPO_OK;
}
// the two networks' arguments for an episode of Nc rows per slot: a.actions / a.logp, c.out are [T][Nc]
static void rec_episode_args(GruFwdArgs &a, GruFwdArgs &c, const float *actor_params, const mappo_net_desc *actor_desc, const float *critic_params,
                             const mappo_net_desc *critic_desc, int Nc, int32_t deterministic, uint64_t seed, uint64_t counter,
                             const uint64_t *counter_dev, float *actions, float *logp, float *values) {
  a.params = actor_params; a.off = net_offsets(*actor_desc); a.desc = *actor_desc; a.L = 1; a.Nc = Nc; a.A = actor_desc->out_dim; a.head_mode = 2;
  a.actions = actions; a.logp = logp; a.deterministic = deterministic; a.seed = seed; a.counter = counter; a.counter_dev = counter_dev;
  c.params = critic_params; c.off = net_offsets(*critic_desc); c.desc = *critic_desc; c.L = 1; c.Nc = Nc; c.A = 1; c.head_mode = 1; c.out = values;
}
