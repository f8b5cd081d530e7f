"""The one-launch rollout episode with the weights in LDS (csrc/mlp_ep16l.h, rollout_episode_lds_kernel; MAPPO_EPISODE_LDS=1):
against the stepwise fused path on the same weights, buffer, env pool and counter, every buffer array and the bootstrap values
must be bit-identical — both run each tile through tile16r_step on the same operands.  Shapes are the smallest that reach each
edge of the kernel: a partial tile, exactly one tile, workgroups whose waves have no item (they must still reach the staging
barrier), many items on one wave, either network squeezed into one workgroup.  Plus the selection rule, which needs no GPU."""
import pytest
import torch

from test_gpu_episode import _assert_same, _runner, _state

REG_VARS = ("MAPPO_EPISODE_WAVES", "MAPPO_EPISODE_NET_WAVES", "MAPPO_EPISODE_INS_WAVES", "MAPPO_EPISODE_COST_A")
LDS_VARS = ("MAPPO_EPISODE_LDS", "MAPPO_EPISODE_LDS_WAVES", "MAPPO_EPISODE_LDS_ACTOR_WGS")


def _clean_env(monkeypatch):
    for k in REG_VARS + LDS_VARS:
        monkeypatch.delenv(k, raising=False)


def _uses_lds(layer_N):
    from mappo_amd import _lib
    return _lib.load().mappo_rollout_episode_uses_lds(layer_N)


def _rollout(episode, monkeypatch, env=None, deterministic=False, n_rollouts=1, **kw):
    _clean_env(monkeypatch)
    monkeypatch.setenv("MAPPO_EPISODE_LDS", "1")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, str(v))
    assert _uses_lds(kw.get("layer_N", 1)) == 1
    r, e = _runner(episode, **kw)
    if deterministic:                                        # the runner samples; argmax goes in at the policy's two entry points
        pol = r.trainer.policy
        step, epi = pol.collect_step_fused, pol.collect_episode_fused
        pol.collect_step_fused = lambda *a, **k: step(*a, deterministic=True, **k)
        pol.collect_episode_fused = lambda *a, **k: epi(*a, deterministic=True, **k)
    states = []
    for _ in range(n_rollouts):
        r.rollout()
        torch.cuda.synchronize()
        states.append(_state(r, e))
    return states


def _check(monkeypatch, envs=({},), **kw):
    ref = _rollout(False, monkeypatch, **kw)
    for env in envs:
        got = _rollout(True, monkeypatch, env=env, **kw)
        for i, (a, b) in enumerate(zip(ref, got)):
            _assert_same(a, b, what=f"{env} rollout {i}: ")
    return ref


NET_CASES = [  # (centralized, layer_N, relu, feature norm, N, M, D, A, T): critic in_dim = M D (centralized) or D
    (True, 1, True, True, 7, 3, 18, 5, 3),          # 21 rows: a partial second tile; critic in_dim 54
    (False, 1, False, False, 7, 3, 18, 5, 3),       # critic in_dim 18, tanh, no feature norm
    (True, 0, True, False, 16, 1, 18, 5, 1),        # exactly one tile, one step
    (False, 0, False, True, 16, 1, 64, 16, 3),      # in_dim 64 (four full k-blocks), out_dim 16 (a full head block)
    (False, 1, True, True, 7, 3, 64, 5, 3),
    (True, 1, False, True, 7, 3, 4, 16, 1),         # in_dim 4: one 16-byte piece per row (critic 12)
    (True, 0, True, True, 7, 3, 4, 5, 3),
    (False, 0, True, False, 7, 3, 18, 16, 1),
]


@pytest.mark.gpu
@pytest.mark.parametrize("centralized,layer_N,relu,fnorm,N,M,D,A,T", NET_CASES)
def test_lds_episode_matches_stepwise(gpu_device, monkeypatch, centralized, layer_N, relu, fnorm, N, M, D, A, T):
    """Two episodes through each path (the second on fresh pool data and a fresh sampling stream)."""
    ref = _check(monkeypatch, centralized=centralized, layer_N=layer_N, relu=relu, fnorm=fnorm, N=N, M=M, D=D, A=A, T=T, n_rollouts=2)
    assert ref[1]["env_t"] == 2 * T


@pytest.mark.gpu
@pytest.mark.parametrize("layer_N,centralized", [(0, True), (1, False)])
def test_lds_episode_more_waves_than_items(gpu_device, monkeypatch, layer_N, centralized):
    """N = 2, M = 3, T = 1: one actor item and two critic items for workgroups of 16 waves (and of 3) — the waves without an item
    stage their share of the weights and pass the barrier (episode16l_body returns nowhere before it)."""
    _check(monkeypatch, envs=({}, {"MAPPO_EPISODE_LDS_WAVES": 3}), layer_N=layer_N, centralized=centralized, N=2, M=3, T=1)


@pytest.mark.gpu
@pytest.mark.parametrize("layer_N", [0, 1])
def test_lds_episode_many_items_per_wave(gpu_device, monkeypatch, layer_N):
    """N = 300, T = 3 (57 tiles, the last partial: 171 actor and 228 critic items) on one wave per workgroup, with the actor's
    share of the workgroups at both ends of its range: one network's items all walk through a single wave."""
    envs = [{"MAPPO_EPISODE_LDS_WAVES": 1, "MAPPO_EPISODE_LDS_ACTOR_WGS": 1}, {"MAPPO_EPISODE_LDS_WAVES": 1, "MAPPO_EPISODE_LDS_ACTOR_WGS": 255},
            {"MAPPO_EPISODE_LDS_WAVES": 1}, {"MAPPO_EPISODE_LDS_WAVES": 5}]
    _check(monkeypatch, envs=envs, layer_N=layer_N, N=300, T=3)


@pytest.mark.gpu
@pytest.mark.parametrize("A", [5, 16])
def test_lds_episode_deterministic_actions(gpu_device, monkeypatch, A):
    ref = _check(monkeypatch, deterministic=True, N=7, A=A, T=3, n_rollouts=2)
    assert ref[0]["actions"].min().item() >= 0 and ref[0]["actions"].max().item() < A


@pytest.mark.gpu
def test_lds_episode_graph_replay(gpu_device, monkeypatch):
    """Eager, capture, two replays: the replays give two different action streams, each the stepwise path's with the same counter."""
    kw = dict(N=64, graph=True, n_rollouts=4)
    ref = _rollout(False, monkeypatch, **kw)
    got = _rollout(True, monkeypatch, **kw)
    for i in range(4):
        _assert_same(ref[i], got[i], what=f"call {i}: ")
    assert not torch.equal(got[2]["actions"], got[3]["actions"])
    assert got[3]["counter"].item() == got[2]["counter"].item() + 25


def test_lds_episode_selection(monkeypatch):
    """layer_N 0 / 1 take the LDS body by default; layer_N 2, MAPPO_EPISODE_LDS=0 and each of the register body's geometry
    overrides (without MAPPO_EPISODE_LDS) take the register body; MAPPO_EPISODE_LDS=1 wins over those overrides."""
    _clean_env(monkeypatch)
    assert [_uses_lds(l) for l in (0, 1, 2)] == [1, 1, 0]
    for k in REG_VARS:
        _clean_env(monkeypatch)
        monkeypatch.setenv(k, "2")
        assert [_uses_lds(l) for l in (0, 1, 2)] == [0, 0, 0], k
        monkeypatch.setenv("MAPPO_EPISODE_LDS", "1")
        assert [_uses_lds(l) for l in (0, 1, 2)] == [1, 1, 0], k
    _clean_env(monkeypatch)
    monkeypatch.setenv("MAPPO_EPISODE_LDS", "0")
    assert [_uses_lds(l) for l in (0, 1, 2)] == [0, 0, 0]
    monkeypatch.setenv("MAPPO_EPISODE_LDS_WAVES", "8")                 # the LDS body's own overrides select nothing
    assert [_uses_lds(l) for l in (0, 1, 2)] == [0, 0, 0]
