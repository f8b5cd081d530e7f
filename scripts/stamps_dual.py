"""Diagnostic (GPU box): per-phase cycles of mlp_update16_dual_kernel (actor + critic in one launch) at the bench shape, from a
-DMLP_STAMPS build.  Builds build_diag/stamps/libmappo_hip_stamps.so (--reuse: keep one that is there) and loads it INSTEAD
of the product library; the product build executes no stamp.

Every wave writes its own stamp row.  For each workgroup the table takes the SLOWEST wave (largest sum of the tile-loop
phases: the one the others wait for at the epilogue's first barrier) and the mean over the network's workgroups; it also
prints the ragged wait (first barrier) of the fastest wave.  Random data and parameters, the bench's shapes
(B = 25 x 1024 x 3 rows, actor 18 -> 5, critic 54 -> 1, layer_N 1), 2 s of back-to-back launches before the stamped one.
usage: python scripts/stamps_dual.py [--reuse] [--json OUT]"""
import ctypes, json, os, sys, time
import torch
sys.path.insert(0, '.')
ROOT = os.getcwd()
objdir = os.path.join(ROOT, 'build_diag', 'stamps')
out = os.path.join(objdir, 'libmappo_hip_stamps.so')
os.makedirs(objdir, exist_ok=True)
if not ('--reuse' in sys.argv and os.path.exists(out)):
    from mappo_amd import build as _build
    _build.build(force=True, verbose=False, extra_flags=['-DMLP_STAMPS', '-w'], lib=out, objdir=objdir)
from mappo_amd import _lib
_lib.LIB_PATH = out
_lib.SIGNATURES['mappo_debug_set_stamps_waves'] = (ctypes.c_int, [ctypes.c_void_p])
from mappo_amd import ops
lib = _lib.load()
NS, NW = 24, 8
NAMES = {0: 'staging + fold', 1: 'xhat0', 2: 'L1 MFMA', 3: 'prefetch + act/LN1', 4: 'L2 MFMA', 5: 'act/LN2',
         6: 'head + loss + head products', 7: 'LN2 bwd + write', 8: 'dW2', 9: 'd xhat1', 10: 'LN1 bwd + write', 11: 'dW1',
         12: 'loop exit', 13: 'first barrier', 18: 'accumulator chunks', 14: 'vector sums', 15: 'raw->grad transform',
         16: 'slab write + partials'}
LOOP = list(range(1, 12))

class A_: pass
a = A_(); a.clip_param=0.2; a.entropy_coef=0.01; a.value_loss_coef=1.0; a.huber_delta=10.0; a.use_huber_loss=True; a.use_clipped_value_loss=True; a.use_policy_active_masks=True; a.use_value_active_masks=True; a.use_valuenorm=True
cfg = ops.ppo_cfg(a)
B = 25 * 1024 * 3
torch.manual_seed(0)
da, dc = ops.net_desc(18, 5), ops.net_desc(54, 1)
Pa, Pc = ops.net_param_count(da), ops.net_param_count(dc)
col_c = ((Pa + 255) // 256) * 256
P = col_c + ((Pc + 255) // 256) * 256
pa = torch.randn(Pa, device='cuda') * 0.1; pc = torch.randn(Pc, device='cuda') * 0.1
obs = torch.randn(B, 18, device='cuda'); sobs = torch.randn(B, 54, device='cuda')
ret = torch.randn(B, device='cuda'); active = (torch.rand(B, device='cuda') > 0.1).float()
mom = torch.zeros(4, dtype=torch.float64, device='cuda'); ops.minibatch_moments(ret, active, None, B, mom)
av = (torch.rand(B, 5, device='cuda') > 0.2).float(); av[:, 0] = 1
act = torch.randint(0, 5, (B,), device='cuda').float(); olp = -torch.rand(B, device='cuda') - 1
adv = torch.randn(B, device='cuda'); vold = torch.randn(B, device='cuda'); vn = torch.tensor([0., 1., 1.], device='cuda')
nd = ops.dual_update_slabs(da, dc, B)
slabs = torch.zeros(nd, P, device='cuda'); pda, pdc = ops.update_partials('cuda'), ops.update_partials('cuda')
stamps = torch.zeros(256 * NW * NS, dtype=torch.int64, device='cuda')      # <= 256 workgroups (mlp_backward_slabs) x 8 waves
assert lib.mappo_debug_set_stamps_waves(ctypes.c_void_p(stamps.data_ptr())) == 0

def run():
    ops.actor_critic_update(pa, da, obs, pc, dc, sobs, None, B, av, act, olp, adv, active, vold, ret, vn, mom, cfg, slabs, P, 0, col_c, pda, pdc)

t_end = time.time() + 2.0
while time.time() < t_end:
    for _ in range(20): run()
    torch.cuda.synchronize()
e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
e0.record()
for _ in range(100): run()
e1.record(); torch.cuda.synchronize()
us = e0.elapsed_time(e1) * 10.0
st = stamps.view(-1, NW, NS).double().cpu()
used = st.sum(2).gt(0).any(1).nonzero().flatten()
n_wg = int(used.max()) + 1
st = st[:n_wg]
res = {'kernel_us_stamped_build': us, 'workgroups': n_wg}
loop = st[:, :, LOOP].sum(2)                                     # [wg][wave]
slow = loop.argmax(1)
fast = loop.argmin(1)
tot = st[:, :, :NS - 1].sum(2)                                   # per wave: the whole body
print(f"stamped build: {us:.1f} us per dual launch (HIP events, 100 launches); {n_wg} workgroups")
nA = int((st[:, 0, NS - 1] == 1).sum())                        # slot 23 holds the body's HEAD (1 actor, 2 critic)
res['nA'] = nA
for name, rows in (('actor', range(0, nA)), ('critic', range(nA, n_wg))):
    rows = list(rows)
    sel = st[rows, slow[rows]]                                   # [wg][phase] of the slowest wave
    m = sel.mean(0)
    wall = tot[rows].max(1).values.mean()
    wait_fast = st[rows, fast[rows], 13].mean()
    print(f"--- {name}: {len(rows)} workgroups; slowest wave per workgroup, mean cycles (whole body {wall:.0f}; "
          f"max over workgroups {tot[rows].max().item():.0f})")
    tab = {}
    for i, n in NAMES.items():
        if m[i] > 0:
            print(f"  {n:30s} {m[i]:9.0f} cyc  {100 * m[i] / wall:5.1f} %")
            tab[n] = float(m[i])
    lp = float(m[LOOP].sum())
    print(f"  {'tile loop (sum)':30s} {lp:9.0f} cyc  {100 * lp / wall:5.1f} %")
    print(f"  {'first barrier, fastest wave':30s} {wait_fast:9.0f} cyc  (ragged wait)")
    tab['tile loop (sum)'] = lp; tab['first barrier, fastest wave'] = float(wait_fast); tab['whole body'] = float(wall)
    res[name] = tab
if '--json' in sys.argv:
    with open(sys.argv[sys.argv.index('--json') + 1], 'w') as f: json.dump(res, f, indent=1)
