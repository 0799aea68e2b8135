"""What the CPU calibration (tests/test_floating_dr_cpu.py) and the GPU tests (tests/test_gpu_floating_dr.py) of FloatingBaseSim's per-env
randomisation share: the per-env draws, one float64 model per env (tests/floating_model.py holds ONE robot's masses, so every env gets its own
model and a batch of one) and the stacked results.  Test-side only."""
import numpy as np

from pbhc_amd.simulator import floating_sim as fsim
from tests import floating_model as fm


def draws(sk, N, seed=17):
    """per env: mass scales in [0.5, 2] on every second body (the root among them), a centre-of-mass bias of up to +-5 cm on one body (the
    one `inertial_table` puts it on), friction in [0.2, 1.2].  -> (names, scale [N,L], bias [N,3], friction [N]) float32"""
    rng = np.random.default_rng(seed)
    names = list(sk.body_names)[:sk.num_bodies][::2]
    scale = rng.uniform(0.5, 2.0, (N, len(names))).astype(np.float32)
    bias = rng.uniform(-0.05, 0.05, (N, 3)).astype(np.float32)
    friction = rng.uniform(0.2, 1.2, N).astype(np.float32)
    return names, scale, bias, friction


def tables(sk, N, seed=17):
    """-> (env_inertial float32 [N,32,4] by the product's own inertial_table, friction float32 [N])"""
    names, scale, bias, friction = draws(sk, N, seed)
    return fsim.FloatingBaseSim.inertial_table(sk, names, scale, bias), friction


def env_models(m, table, friction):
    """one model per env: the nominal model with the env's row of the table (its float32 values) and the env's friction"""
    B = m["B"]
    return [dict(m, mass=table[n, :B, 0].astype(np.float64), com=table[n, :B, 1:].astype(np.float64), friction=float(np.float32(friction[n])))
            for n in range(len(table))]


def forward_each(models, root, q, v, tau, h, dtype=np.float64):
    """fm.forward of env n's model on row n (a batch of one), stacked -> acc [N,6+D], f [N,K,3], dict(terms, f_abs, z, J)"""
    acc, f, keep = [], [], {k: [] for k in ("terms", "f_abs", "z", "J")}
    for n, m in enumerate(models):
        sl = slice(n, n + 1)
        a, ff, d = fm.forward(m, fm.state(root[sl], q[sl], v[sl], dtype), tau[sl], h, dtype)
        acc.append(a); f.append(ff)
        for k in keep:
            keep[k].append(d[k])
    return np.concatenate(acc, 0), np.concatenate(f, 0), {k: np.concatenate(x, 0) for k, x in keep.items()}
