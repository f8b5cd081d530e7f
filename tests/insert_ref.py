"""NumPy restatement of the rollout inserts, written from the reference's Python and independent of the HIP kernels: the
runners' insert() (onpolicy/runner/shared/mpe_runner.py:125-139, smac_runner.py:129-151) followed by the slot writes of
SharedReplayBuffer.insert (onpolicy/utils/shared_buffer.py:74-112).  No torch.  Every function takes plain contiguous
arrays and returns the arrays the reference writes into the buffer slots of one step (obs, share_obs, masks, bad_masks,
active_masks, available_actions and the rnn states go to slot step + 1, rewards to slot step).

One deliberate difference, which the project's kernels and its earlier tests share: where the reference assigns zeros to the
rnn states of a finished row, the slot value here is the float32 product state * keep with keep = 1 - done.  The two agree on
every finite state except in the sign of the zero (-x * 0 = -0.0); inf * 0 and NaN * 0 are NaN.  tests/test_oracle_golden.py
pins these functions against tests/golden/insert.npz, which the reference wrote."""
import numpy as np

F32 = np.float32


def _keep(done):
    """1 - done as float32, the reference's masks[dones == True] = 0 on an array of ones."""
    keep = np.ones(done.shape, dtype=F32)
    keep[np.asarray(done, dtype=bool)] = 0.0
    return keep


def _masked(states, keep_rows):
    """states [R, ...] * keep_rows [R] in float32 (see the module docstring)."""
    s = np.asarray(states, dtype=F32)
    with np.errstate(invalid="ignore"):
        return s * keep_rows.reshape((-1,) + (1,) * (s.ndim - 1)).astype(F32)


def insert_mpe_ref(obs, rewards, dones, centralized, rnn=None):
    """obs [N, M, D] float32, rewards [N, M] or [N, M, 1], dones [N, M] bool; rnn: None or (rnn_states, rnn_states_critic),
    each [N * M, ...].  Returns (obs_slot [N, M, D], share_slot [N, M, M * D | D], rew_slot [N, M, 1], mask_slot [N, M, 1]),
    followed by (rnn_slot, rnn_critic_slot) in the shapes given when rnn is not None."""
    obs = np.asarray(obs, dtype=F32)
    N, M, D = obs.shape
    dones = np.asarray(dones, dtype=bool).reshape(N, M)
    masks = _keep(dones).reshape(N, M, 1)
    if centralized:                                             # mpe_runner.py:133-135
        share_obs = obs.reshape(N, -1)
        share_obs = np.expand_dims(share_obs, 1).repeat(M, axis=1)
    else:
        share_obs = obs
    out = (obs.copy(), share_obs.copy(), np.asarray(rewards, dtype=F32).reshape(N, M, 1).copy(), masks)
    if rnn is not None:
        keep = masks.reshape(N * M)
        out += (_masked(rnn[0], keep), _masked(rnn[1], keep))
    return out


def insert_smac_ref(obs, share_obs, avail, rewards, dones, bad_transition=None, rnn=None):
    """obs [N, M, D], share_obs [N, M, S], avail [N, M, A] or None, rewards [N, M(, 1)], dones [N, M] bool, bad_transition
    [N, M] bool or None (no bad transitions), rnn: None or (rnn_states, rnn_states_critic), each [N * M, ...].
    Returns the nine slot arrays (obs, share_obs, available_actions, rewards, masks, bad_masks, active_masks, rnn_states,
    rnn_states_critic); available_actions and the two state arrays are None where their source is None."""
    obs = np.asarray(obs, dtype=F32)
    N, M, _ = obs.shape
    dones = np.asarray(dones, dtype=bool).reshape(N, M)
    dones_env = np.all(dones, axis=1)                           # smac_runner.py:133
    masks = np.ones((N, M, 1), dtype=F32)
    masks[dones_env] = 0.0
    active_masks = np.ones((N, M, 1), dtype=F32)
    active_masks[dones] = 0.0
    active_masks[dones_env] = 1.0
    bad_masks = np.ones((N, M, 1), dtype=F32)
    if bad_transition is not None:
        bad_masks[np.asarray(bad_transition, dtype=bool).reshape(N, M)] = 0.0
    ha = hc = None
    if rnn is not None:
        keep = np.repeat(masks.reshape(N, M)[:, :1], M, axis=1).reshape(N * M)      # per env, every agent
        ha, hc = _masked(rnn[0], keep), _masked(rnn[1], keep)
    return (obs.copy(), np.asarray(share_obs, dtype=F32).copy(), None if avail is None else np.asarray(avail, dtype=F32).copy(),
            np.asarray(rewards, dtype=F32).reshape(N, M, 1).copy(), masks, bad_masks, active_masks, ha, hc)


def episode_insert_ref(env_obs, rewards, dones, centralized):
    """The MPE insert of every step of an episode: env_obs [T, N, M, D], rewards [T, N, M(, 1)], dones [T, N, M] bool.
    Returns (obs_buf[1:], share_buf[1:], rew_buf, mask_buf[1:]) = ([T, N, M, D], [T, N, M, S], [T, N, M, 1], [T, N, M, 1]):
    step t's env output goes to slot t + 1 of obs / share_obs / masks and to slot t of rewards."""
    T = np.asarray(env_obs).shape[0]
    rewards = np.asarray(rewards, dtype=F32).reshape(np.asarray(dones).shape)
    steps = [insert_mpe_ref(env_obs[t], rewards[t], dones[t], centralized) for t in range(T)]
    return tuple(np.stack([s[k] for s in steps]) for k in range(4))
