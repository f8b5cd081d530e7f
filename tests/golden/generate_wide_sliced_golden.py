"""Writes tests/golden/wide_sliced_parent.npz: the outputs of mappo_mlp_forward and mappo_actor_update at in_dim 65 and 512, as
the library computed them on the MI355X BEFORE in_dim 513..2048 was admitted (the commit that still had MAPPO_MAX_IN_DIM 512).
tests/test_gpu_wide_sliced.py::test_unchanged_below_limit repeats the calls and compares bit for bit: the widths up to 512
keep their kernels and launch sequences.

Run on a GPU machine from the repository root, on the commit whose outputs are to be pinned:

    python tests/golden/generate_wide_sliced_golden.py [output.npz [commit hash]]

The committed file was written on commit 732b3d4 ("Run MPE simple_world_comm's rollout episode in one launch (opt-in)"), the parent
of the change that moved the limit; the hash of the producing commit is stored in the file under `meta/commit` (taken from git
where the script runs, or from the second argument).

cases() is imported by the test, so both sides build the same inputs."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
A, LN, RELU, FN = 5, 1, True, True
WIDTHS = (65, 512)
B_FWD, B_UPD = 40, 17


def cases(n_params):
    """{D: dict of host arrays}; n_params(D) = parameter count of the actor descriptor."""
    out = {}
    for D in WIDTHS:
        rng = np.random.default_rng(1000 + D)
        f = np.float32
        P = n_params(D)
        n_rows = B_FWD + 8
        c = dict(params=(rng.standard_normal(P) * 0.1).astype(f), x=rng.standard_normal((n_rows, D)).astype(f),
                 rows_fwd=rng.permutation(n_rows)[:B_FWD].astype(np.int32), rows_upd=rng.permutation(n_rows)[:B_UPD].astype(np.int32))
        avail = (rng.random((n_rows, A)) > 0.3).astype(f)
        actions = rng.integers(0, A, n_rows).astype(f)
        avail[np.arange(n_rows), actions.astype(int)] = 1.0
        c.update(avail=avail, actions=actions, old_logp=(-np.abs(rng.standard_normal(n_rows)) * 0.3 - np.log(A)).astype(f),
                 adv=rng.standard_normal(n_rows).astype(f), active=(rng.random(n_rows) > 0.25).astype(f),
                 ret=rng.standard_normal(n_rows).astype(f))
        out[D] = c
    return out


def run(ops, torch, args):
    """{name: array}: logits of mlp_forward (gathered rows) and the slab / loss partials of actor_update at every width."""
    res = {}
    cs = cases(lambda D: ops.net_param_count(ops.net_desc(D, A, LN, RELU, FN)))
    cfg = ops.ppo_cfg(args)
    for D, c in cs.items():
        d = ops.net_desc(D, A, LN, RELU, FN)
        g = {k: torch.from_numpy(v).cuda() for k, v in c.items()}
        logits = torch.zeros(B_FWD, A, device="cuda")
        ops.mlp_forward(g["params"], d, g["x"], g["rows_fwd"], B_FWD, logits)
        res[f"d{D}/logits"] = logits.cpu().numpy()
        P = int(g["params"].numel())
        ns = ops.mlp_backward_slabs(B_UPD)
        slabs = torch.zeros(ns, P, device="cuda")
        part = ops.update_partials("cuda")
        mom = torch.zeros(4, dtype=torch.float64, device="cuda")
        ops.minibatch_moments(g["ret"], g["active"], g["rows_upd"], B_UPD, mom)
        ops.actor_update(g["params"], d, g["x"], g["rows_upd"], B_UPD, g["avail"], g["actions"], g["old_logp"], g["adv"], g["active"], mom,
                         cfg, slabs, P, 0, part)
        torch.cuda.synchronize()
        res[f"d{D}/slabs"] = slabs.cpu().numpy()
        res[f"d{D}/partials"] = part.cpu().numpy()[:4 * ns]
    return res


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import torch
    from mappo_amd import ops
    from oracle import mappo_oracle as O
    dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(HERE, "wide_sliced_parent.npz")
    os.makedirs(os.path.dirname(os.path.abspath(dst)), exist_ok=True)
    if len(sys.argv) > 2:
        commit = sys.argv[2]
    else:
        import subprocess
        commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=HERE, capture_output=True, text=True).stdout.strip() or "unknown"
    np.savez_compressed(dst, **run(ops, torch, O.default_args()), **{"meta/commit": np.array(commit)})
    print("wrote", dst)
