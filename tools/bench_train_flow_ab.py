"""cfg-4 SU(3) train step (8^4, 256 chains, nleapfrog 4, units [256]) with the clover charge at flow time 0 and 0.1
(eps 0.02): two trainers alternating in one process, device-synchronised host clock around 5 steps, 4 repetitions."""
import os, sys, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'l2hmc-qcd_amd'))
import l2hmc.configs as cfgs
from l2hmc.trainers.pytorch.trainer import Trainer

BASE = ['dynamics.group=SU3', 'dynamics.latvolume=[8,8,8,8]', 'dynamics.nchains=256', 'dynamics.nleapfrog=4',
        'dynamics.eps=0.01', 'dynamics.verbose=false', 'dynamics.use_split_xnets=false',
        'dynamics.use_separate_networks=false', 'network.units=[256]', 'network.activation_fn=tanh',
        'network.dropout_prob=0.0', 'network.use_batch_norm=false', 'conv=none', 'loss.plaq_weight=0.1',
        'loss.rmse_weight=0.1', 'loss.charge_weight=0.01', 'loss.charge_kind=clover', 'loss.charge_flow_eps=0.02']
CASES = {'flow_time=0': ['loss.charge_flow_time=0.0'], 'flow_time=0.1': ['loss.charge_flow_time=0.1']}
trainers, xs = {}, {}
for name, ov in CASES.items():
    torch.manual_seed(9992); np.random.seed(9992)
    trainers[name] = Trainer(cfgs.get_config(BASE + ov))
    xs[name] = trainers[name].lattice.random()
    xs[name], _ = trainers[name].train_step((xs[name], 6.0))           # warm-up
times = {k: [] for k in CASES}
for rep in range(4):
    for name, tr in trainers.items():
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(5):
            xs[name], m = tr.train_step((xs[name], 6.0))
        torch.cuda.synchronize()
        times[name].append((time.perf_counter() - t0) / 5 * 1e3)
        print(f'{name} rep {rep}: {times[name][-1]:.2f} ms/step loss={m["loss"]:.4g}', flush=True)
for name, t in times.items():
    print(f'{name}: ' + ', '.join(f'{v:.2f}' for v in t) + f'  median {np.median(t):.2f} ms/step', flush=True)
print(f'peak mem {torch.cuda.max_memory_allocated() / 2**30:.1f} GiB')
