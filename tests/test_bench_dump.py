"""bench.py --dump-outputs on host tensors: a fixed, seeded sample of the envs when the whole rollout would not fit, float32 / float64
files only, at most 64 MB in all, and the same files from run to run."""
import types

import numpy as np
import torch

import bench
from pbhc_amd.agents.modules import RolloutStorage


def _agent(T, N, obs_dims, seed=0):
    g = torch.Generator().manual_seed(seed)
    st = RolloutStorage(N, T, "cpu")
    for k, d in obs_dims.items():
        st.register_key(k, shape=(d,), pad_rows=True, tail_slab=True)
    for k, d in (("actions", 23), ("rewards", 20), ("values", 20), ("returns", 20), ("advantages", 1)):
        st.register_key(k, shape=(d,))
    st.register_key("dones", shape=(1,), dtype=torch.bool)
    for k in st.stored_keys:
        t = st.with_tail(k) if k in obs_dims else getattr(st, k)
        t.copy_(torch.rand(t.shape, generator=g) > 0.5 if t.dtype == torch.bool else torch.randn(t.shape, generator=g))
    obs = {k: st.with_tail(k)[T] for k in obs_dims}
    torch.manual_seed(seed)
    algo = types.SimpleNamespace(storage=st, actor=torch.nn.Linear(obs_dims["actor_obs"], 23), critic=torch.nn.Linear(obs_dims["critic_obs"], 20))
    return algo, obs, {"Value": torch.tensor(0.25), "Surrogate": torch.tensor(-0.5, dtype=torch.float64)}


def test_dump_samples_envs_within_the_budget(tmp_path):
    T, N = 24, 256
    algo, obs, losses = _agent(T, N, {"actor_obs": 38, "critic_obs": 63})
    bench.dump_outputs(algo, obs, losses, str(tmp_path / "a"), max_envs=64)
    bench.dump_outputs(algo, obs, losses, str(tmp_path / "b"), max_envs=64)
    files = sorted(p.name for p in (tmp_path / "a").iterdir())
    assert files == sorted(p.name for p in (tmp_path / "b").iterdir())
    a = {f[:-4]: np.load(tmp_path / "a" / f) for f in files}
    for f in files:
        assert np.array_equal(a[f[:-4]], np.load(tmp_path / "b" / f)), f
    assert all(x.dtype in (np.float32, np.float64) for x in a.values())
    idx = np.sort(np.random.default_rng(0).choice(N, 64, replace=False))
    assert a["obs.actor_obs"].shape == (64, 38) and a["rollout.rewards"].shape == (T, 64, 20) and a["rollout.dones"].dtype == np.float32
    assert np.array_equal(a["obs.critic_obs"], obs["critic_obs"][idx].numpy())
    assert np.array_equal(a["rollout.returns"], algo.storage.returns[:, idx].numpy())
    assert np.array_equal(a["rollout.dones"], algo.storage.dones[:, idx].float().numpy())
    assert a["loss.Surrogate"].dtype == np.float64 and a["loss.Value"] == np.float32(0.25)
    assert np.array_equal(a["param.actor.weight"], algo.actor.weight.detach().numpy())
    assert "param.critic.bias" in a and not any(k.startswith("rollout.actor_obs") for k in a)


def test_dump_halves_the_sample_until_it_fits(tmp_path, monkeypatch):
    T, N = 24, 256
    algo, obs, losses = _agent(T, N, {"actor_obs": 38, "critic_obs": 63})
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 200_000)
    bench.dump_outputs(algo, obs, losses, str(tmp_path))
    a = {p.name[:-4]: np.load(p) for p in tmp_path.iterdir()}
    assert sum(x.nbytes for x in a.values()) <= 200_000
    # per env 4 * (38 + 63 + 24 * 85) = 8 564 bytes, weights and losses 8 720: 256, 128, 64 and 32 envs do not fit, 16 do
    assert a["obs.critic_obs"].shape == (16, 63)
