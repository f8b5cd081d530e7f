"""The episode kernel deals each network's (step, tile) items over its waves (csrc/mlp_fwd16.h episode16r_body, geometry in
mappo_rollout_episode).  The edges of that distribution — one step, item counts that the wave count does not divide, fewer items
than waves, many items per wave, every geometry override — each bit-identical to the stepwise path on the same weights, buffer,
env pool and counter."""
import pytest
import torch

from test_gpu_episode import _assert_same, _runner, _state

GEOM_VARS = ("MAPPO_EPISODE_WAVES", "MAPPO_EPISODE_NET_WAVES", "MAPPO_EPISODE_INS_WAVES", "MAPPO_EPISODE_COST_A")


def _rollout(episode, geom, monkeypatch, **kw):
    for k in GEOM_VARS:
        monkeypatch.delenv(k, raising=False)
    for k, v in geom.items():
        monkeypatch.setenv(k, str(v))
    r, env = _runner(episode, **kw)
    r.rollout()
    torch.cuda.synchronize()
    return _state(r, env)


def _check(monkeypatch, geoms, **kw):
    ref = _rollout(False, {}, monkeypatch, **kw)
    for g in geoms:
        _assert_same(ref, _rollout(True, g, monkeypatch, **kw), what=f"{g}: ")


@pytest.mark.gpu
@pytest.mark.parametrize("centralized", [True, False])
def test_episode_one_step(gpu_device, monkeypatch, centralized):
    """T = 1: the actor has one step, the critic two (the second is the bootstrap)."""
    _check(monkeypatch, [{}, {"MAPPO_EPISODE_NET_WAVES": 3}], centralized=centralized, N=100, T=1)


@pytest.mark.gpu
def test_episode_items_not_dividing_waves(gpu_device, monkeypatch):
    """N = 1000 (188 tiles, the last partial): 4 700 / 4 888 items over wave counts that divide neither."""
    _check(monkeypatch, [{"MAPPO_EPISODE_NET_WAVES": 7}, {"MAPPO_EPISODE_NET_WAVES": 13, "MAPPO_EPISODE_WAVES": 4},
                         {"MAPPO_EPISODE_NET_WAVES": 997, "MAPPO_EPISODE_WAVES": 2}], N=1000)


@pytest.mark.gpu
@pytest.mark.parametrize("T", [1, 25])
def test_episode_fewer_items_than_waves(gpu_device, monkeypatch, T):
    """N = 1 (one partial tile of 3 rows): T or T + 1 items per network against the default 1 024 waves."""
    _check(monkeypatch, [{}, {"MAPPO_EPISODE_WAVES": 4}, {"MAPPO_EPISODE_INS_WAVES": 5}], N=1, T=T)


@pytest.mark.gpu
def test_episode_many_items_per_wave(gpu_device, monkeypatch):
    """N = 8 192 (1 536 tiles): ~38 items per wave at the default geometry, and every item of a network on one wave."""
    _check(monkeypatch, [{}, {"MAPPO_EPISODE_NET_WAVES": 2}], N=8192)


GEOMS = [
    {"MAPPO_EPISODE_WAVES": 1},
    {"MAPPO_EPISODE_WAVES": 2},
    {"MAPPO_EPISODE_WAVES": 4},
    {"MAPPO_EPISODE_NET_WAVES": 512},
    {"MAPPO_EPISODE_INS_WAVES": 128},
    {"MAPPO_EPISODE_INS_WAVES": 256, "MAPPO_EPISODE_WAVES": 4},
    {"MAPPO_EPISODE_COST_A": 1},
    {"MAPPO_EPISODE_COST_A": 1000},
]


@pytest.mark.gpu
@pytest.mark.parametrize("layer_N,relu,fnorm", [(1, True, True), (2, False, False)])
def test_episode_every_geometry(gpu_device, monkeypatch, layer_N, relu, fnorm):
    """The bench shape (N = 1 024, centralized critic) under every geometry override."""
    _check(monkeypatch, GEOMS, layer_N=layer_N, relu=relu, fnorm=fnorm, N=1024)
