"""CPU: mappo_actor_critic_update_group / mappo_reduce_clip_adam_group (include/mappo_hip.h) refuse what they do not serve with
MAPPO_EINVAL and a message that names the job — before any launch, so fake non-NULL pointers do and no GPU is needed."""
import ctypes as C

import pytest

from mappo_amd import _lib

FAKE = 4096                                  # non-NULL, never dereferenced: the checks come before any launch


def _desc(in_dim=10, out_dim=5, layer_N=1, use_relu=1, fn=1, recurrent=0):
    return _lib.NetDesc(in_dim, 64, out_dim, layer_N, use_relu, fn, recurrent)


def _job(actor=None, critic=None, **kw):
    j = _lib.UpdateJob()
    for name, typ in _lib.UpdateJob._fields_:
        if typ is C.c_void_p:
            setattr(j, name, FAKE)
    j.actor_desc = actor or _desc()
    j.critic_desc = critic or _desc(28, 1, j.actor_desc.layer_N, j.actor_desc.use_relu, j.actor_desc.use_feature_norm)
    j.cfg = _lib.PpoCfg(0.2, 0.01, 1.0, 10.0, 1, 1, 1, 1, 1, 0)
    j.B, j.slab_stride, j.actor_col0, j.critic_col0 = 40, 1 << 20, 0, 1 << 19
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _opt_job(**kw):
    j = _lib.OptimJob()
    for name, typ in _lib.OptimJob._fields_:
        if typ is C.c_void_p:
            setattr(j, name, FAKE)
    j.n_slabs, j.slab_stride, j.n_seg = 3, 1 << 20, 2
    for s, b in enumerate((0, 5120, 12032)):
        j.seg_bounds[s] = b
    for k, v in kw.items():
        setattr(j, k, v)
    return j


def _update(jobs, n=None):
    lib = _lib.load()
    arr = (_lib.UpdateJob * len(jobs))(*jobs) if jobs else None
    rc = lib.mappo_actor_critic_update_group(arr, len(jobs) if n is None else n, None)
    return rc, lib.mappo_last_error().decode()


def _optim(jobs, n=None):
    lib = _lib.load()
    arr = (_lib.OptimJob * len(jobs))(*jobs) if jobs else None
    rc = lib.mappo_reduce_clip_adam_group(arr, len(jobs) if n is None else n, None)
    return rc, lib.mappo_last_error().decode()


def test_abi_and_limits():
    assert _lib.load().mappo_abi_version() >= 14 and _lib.MAX_GROUP == 8


@pytest.mark.parametrize("call,who,make", [(_update, "actor_critic_update_group", _job), (_optim, "reduce_clip_adam_group", _opt_job)])
def test_job_count_and_null_array(call, who, make):
    for n in (0, 9, -1):
        rc, msg = call([make() for _ in range(9)], n)
        assert rc == -1 and who in msg and f"n_jobs={n}" in msg and "job" in msg, msg
    rc, msg = call([], 3)
    assert rc == -1 and who in msg and "null job array" in msg and "job 0" in msg, msg


UPDATE_REFUSALS = [
    ("in_dim 65", lambda: [_job(), _job(actor=_desc(65))], ("job 1", "in_dim 65")),
    ("critic in_dim 65", lambda: [_job(critic=_desc(65, 1))], ("job 0", "in_dim 65")),
    ("recurrent", lambda: [_job(), _job(), _job(actor=_desc(recurrent=1), critic=_desc(28, 1, recurrent=1))], ("job 2", "recurrent")),
    ("recurrent critic", lambda: [_job(critic=_desc(28, 1, recurrent=1)), _job()], ("job 0", "recurrent")),
    ("layer_N 2", lambda: [_job(), _job(actor=_desc(layer_N=2))], ("job 1", "layer_N 2")),
    ("out_dim 17", lambda: [_job(actor=_desc(out_dim=17)), _job()], ("job 0", "out_dim 17")),
    ("use_relu differs", lambda: [_job(), _job(), _job(), _job(actor=_desc(use_relu=0))], ("job 3", "use_relu 0", "job 0")),
    ("layer_N differs", lambda: [_job(), _job(actor=_desc(layer_N=0))], ("job 1", "layer_N 0", "job 0")),
    ("feature norm differs", lambda: [_job(), _job(actor=_desc(fn=0))], ("job 1", "use_feature_norm", "job 0")),
    ("pair-kernel actor", lambda: [_job(), _job(actor=_desc(in_dim=40, layer_N=1))], ("job 1", "pair kernel")),
    ("null pointer", lambda: [_job(), _job(adv=None)], ("job 1", "null pointer")),
    ("valuenorm without state", lambda: [_job(vn_state=None)], ("job 0", "vn_state")),
    ("B = 0", lambda: [_job(), _job(B=0)], ("job 1", "B=0")),
    ("slab columns", lambda: [_job(), _job(slab_stride=1000)], ("job 1", "slab column range")),
    ("hidden 128", lambda: [_job(actor=_lib.NetDesc(10, 128, 5, 1, 1, 1, 0))], ("job 0", "hidden_size")),
]


@pytest.mark.parametrize("name,jobs,words", UPDATE_REFUSALS, ids=[c[0] for c in UPDATE_REFUSALS])
def test_update_group_refuses_by_job(name, jobs, words):
    rc, msg = _update(jobs())
    assert rc == -1 and "actor_critic_update_group" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_wide_actor_without_hidden_layer_is_a_job_the_dual_kernel_serves():
    """33..64 inputs with layer_N = 0 is a 16-sample-tile shape: the refusal of job 1 below is about ITS pointer, not job 0's width."""
    rc, msg = _update([_job(actor=_desc(in_dim=40, layer_N=0)), _job(actor=_desc(layer_N=0), obs=None)])
    assert rc == -1 and "job 1" in msg and "null pointer" in msg, msg


OPTIM_REFUSALS = [
    ("null pointer", lambda: [_opt_job(), _opt_job(grad=None)], ("job 1", "null pointer")),
    ("n_seg", lambda: [_opt_job(n_seg=5)], ("job 0", "n_seg=5")),
    ("n_slabs", lambda: [_opt_job(), _opt_job(), _opt_job(n_slabs=0)], ("job 2", "n_slabs=0")),
    ("stride", lambda: [_opt_job(), _opt_job(slab_stride=256)], ("job 1", "slab_stride")),
]


@pytest.mark.parametrize("name,jobs,words", OPTIM_REFUSALS, ids=[c[0] for c in OPTIM_REFUSALS])
def test_optim_group_refuses_by_job(name, jobs, words):
    rc, msg = _optim(jobs())
    assert rc == -1 and "reduce_clip_adam_group" in msg, msg
    for w in words:
        assert w in msg, (w, msg)


def test_optim_group_refuses_bad_segment_bounds():
    j = _opt_job()
    j.seg_bounds[1] = 5000                                           # not a multiple of 256
    rc, msg = _optim([_opt_job(), j])
    assert rc == -1 and "job 1" in msg and "multiples of 256" in msg, msg
    j = _opt_job()
    j.seg_bounds[0] = 256
    rc, msg = _optim([j])
    assert rc == -1 and "job 0" in msg and "seg_bounds[0]" in msg, msg
