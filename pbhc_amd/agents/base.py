"""What MHPPO (agents/mh_ppo.py) and ppo_mimic.PPO (agents/ppo_mimic.py) both are: an agent whose whole training iteration stays on the device.

`OnDeviceAgent` owns the constructor body, `setup()`, the learn loop, GAE, the registration of the rollout buffer's common keys and of the update's
scratch buffers, the logging and the frame of `_training_step`; `FlatAdamView` is the torch.optim-format checkpoint view of the flat Adam
buffers.  The rollout itself is agents/rollout.py.  The run-time switches of INTEGRATION.md that concern the agents are read here (`switch`).
"""
from __future__ import annotations

import os

import torch

from .. import _lib
from .. import dist as pdist
from ..utils import resume, rng_state
from .modules import RolloutStorage

# name -> default.  Read at the time of use, not at import: the tests flip them between two agents of one process.
SWITCHES = {"PBHC_ROLLOUT_GRAPH": "1", "PBHC_ROLLOUT_SPLIT": "1", "PBHC_CRITIC_BATCHED": "1", "PBHC_FUSED_SAMPLE": "1", "PBHC_STACK_NETS": "actor",
            "PBHC_STACK_NETS_V2": "1", "PBHC_FWD_GRAPHS": "1", "PBHC_PERM_PREFETCH": "1", "PBHC_CHECK_GRAD_CLEAN": "0", "PBHC_ASSEMBLE_INPUTS": "1",
            "PBHC_ROLLOUT_RIDERS": "1", "PBHC_PAIR_TAILS": "1", "PBHC_PAIR_WIDE": "1", "PBHC_STEP_FINISH": "1"}


def switch(name):
    """the value of a run-time switch (a string)"""
    return os.environ.get(name, SWITCHES[name])


def switch_on(name):
    """an on / off switch: one that defaults to on is turned off by "0", one that defaults to off is turned on by "1" """
    return switch(name) != "0" if SWITCHES[name] == "1" else switch(name) == "1"


class _NullWriter:
    def __getattr__(self, n):
        return lambda *a, **k: None


def _make_writer(log_dir):
    if log_dir is None:
        return _NullWriter()
    try:
        from torch.utils.tensorboard import SummaryWriter

        return SummaryWriter(log_dir=log_dir, flush_secs=10)
    except Exception:
        return _NullWriter()


class PhaseTimer:
    """`Perf/collection_time` / `Perf/learning_time` (mh_ppo.py:223-230,325-327) as DEVICE time.  The reference's host clock deltas mean
    "time the phase took" only because its rollout synchronises with the host every step; an iteration here is fully asynchronous, so the
    phases are bracketed by HIP events on the compute stream and read back when a logging interval ends (one synchronisation per
    interval, none per iteration)."""

    def __init__(self):
        self._cur, self._pending = None, []

    def start(self):
        e = torch.cuda.Event(enable_timing=True)
        e.record()
        self._cur = [e]

    def split(self):
        """end of the phase that started at the previous mark (no-op outside learn())"""
        if self._cur is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record()
            self._cur.append(e)
            if len(self._cur) == 3:
                self._pending.append(self._cur)
                self._cur = None

    def resolve(self):
        """-> [(collection_s, learn_s)] of the iterations finished since the last call (synchronises on the last one)."""
        out = []
        if self._pending:
            self._pending[-1][2].synchronize()
            out = [(a.elapsed_time(b) * 1e-3, b.elapsed_time(c) * 1e-3) for a, b, c in self._pending]
            self._pending = []
        return out


def _load_checkpoint(path, device):
    """Checkpoints — ours, the reference's, a third party's `model_*.pt` — hold tensors, numbers, strings, tuples, lists, dicts and None
    (state dicts, torch.optim state, `iter`, `infos`): they are read with the non-executing loader only.  A file that needs more than
    that is refused, never unpickled."""
    try:
        return torch.load(path, map_location=device, weights_only=True)
    except Exception as e:          # pickle.UnpicklingError / RuntimeError from the restricted unpickler
        raise _lib.PbhcError(f"checkpoint {path}: not loadable with torch.load(weights_only=True) ({type(e).__name__}: {str(e)[:300]}); "
                             "pbhc_amd does not unpickle arbitrary objects — re-save the file with plain tensors / numbers in `infos`") from e


class FlatAdamView:
    """torch.optim.Adam / AdamW-format state_dict()/load_state_dict() over some parameters of the flat Adam buffers, so that checkpoints keep the
    reference's `*optimizer_state_dict` entries (mh_ppo.py:195-204, ppo_mimic.py:237-265).
    entries: [(offset, numel, shape, stepped)] in the optimiser's parameter order (stepped False: a parameter this optimiser never has a
    gradient for — torch keeps no state for it); m / v: the moment buffers; step / lr: one-element views of the step count and of the learning
    rate (a wider `lr` is filled on load; load_lr False: the learning rate is not read back).  keep_unstepped: write the (zero) state of an optimiser that has not stepped yet as well."""

    def __init__(self, algo, entries, m, v, step, lr, weight_decay=0, keep_unstepped=False, load_lr=True):
        self.algo, self.entries, self.m, self.v, self.step, self.lr = algo, entries, m, v, step, lr
        self.weight_decay, self.keep_unstepped, self.load_lr = weight_decay, keep_unstepped, load_lr

    def state_dict(self):
        a, state = self.algo, {}
        if self.keep_unstepped or float(self.step[0]) > 0:
            for i, (o, k, shape, stepped) in enumerate(self.entries):
                if stepped:
                    state[i] = {"step": self.step[0].detach().clone().cpu(), "exp_avg": self.m[o:o + k].view(shape).clone(),
                                "exp_avg_sq": self.v[o:o + k].view(shape).clone()}
        group = {"lr": float(self.lr[0]), "betas": tuple(a.betas), "eps": a.adam_eps, "weight_decay": self.weight_decay, "amsgrad": False,
                 "maximize": False, "foreach": None, "capturable": False, "differentiable": False, "fused": None,
                 "params": list(range(len(self.entries)))}
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, sd):
        for i, (o, k, _, _) in enumerate(self.entries):
            if i in sd["state"]:
                e = sd["state"][i]
                self.m[o:o + k].copy_(e["exp_avg"].reshape(-1).to(self.algo.device))
                self.v[o:o + k].copy_(e["exp_avg_sq"].reshape(-1).to(self.algo.device))
                self.step[0] = float(e["step"])
        if self.load_lr:
            self.lr[:] = float(sd["param_groups"][0]["lr"])

    @property
    def param_groups(self):
        return [{"lr": float(self.lr[0])}]


class OnDeviceAgent:
    """Base of the two agents.  A subclass provides `_init_config` (extending the one here), `_setup_models_and_optimizer`, `_setup_storage`,
    `_rollout_step`, `_training_step`, `_critic_values`, `_log_scalars`, `_log_line`, `save`."""

    def __init__(self, env, config, log_dir=None, device="cpu"):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _lib.PbhcError(f"{type(self).__module__}.{type(self).__name__} runs on the GPU only")
        self.env = env
        self.config = config
        self.log_dir = log_dir
        self.writer = _make_writer(log_dir)
        self.collection_time = self.learn_time = 0
        self._timer = PhaseTimer()
        self._init_config()
        self.tot_timesteps = 0
        self.tot_time = 0
        self.current_learning_iteration = 0
        self.ep_infos = []
        N = self.env.num_envs
        self.cur_reward_sum = torch.zeros(N, dtype=torch.float, device=self.device)
        self.cur_episode_length = torch.zeros(N, dtype=torch.float, device=self.device)
        # device-side episode statistics: [sum of returns, sum of lengths, count] of finished episodes
        self._ep_stats = torch.zeros(3, dtype=torch.float64, device=self.device)
        self.world_size, self.rank = pdist.world(), pdist.rank()
        self._dp = pdist.active()                    # data-parallel exchanges on (more than one rank, or a forced one-rank rehearsal)
        # algo.config.sync_env_statistics: "rollout" (default; True means the same) | "step" (exact single-process equivalence) | False
        self._stat_mode = {True: "rollout", False: None, None: None}.get(config.get("sync_env_statistics", "rollout"), config.get("sync_env_statistics", "rollout"))
        if self._dp and self._stat_mode and hasattr(self.env, "enable_global_statistics"):
            self.env.enable_global_statistics(mode=self._stat_mode)     # sigma / episode-length curricula from the batch of all ranks' envs
        _ = self.env.reset_all()

    def _init_config(self):
        c = self.config
        self.num_envs = self.env.num_envs
        self.algo_obs_dim_dict = self.env.config.robot.algo_obs_dim_dict
        self.num_act = self.env.config.robot.actions_dim
        self.num_rew_fn = self.env.num_rew_fn
        self.logging_interval = c.get("logging_interval", 10)
        for k in ("save_interval", "num_steps_per_env", "load_optimizer", "num_learning_iterations", "init_at_random_ep_len", "desired_kl", "schedule",
                  "clip_param", "num_learning_epochs", "num_mini_batches", "gamma", "lam", "value_loss_coef", "entropy_coef", "max_grad_norm",
                  "use_clipped_value_loss"):
            setattr(self, k, c[k])

    def setup(self):
        from .gemm_tuning import enable as _enable_gemm_tuning

        _enable_gemm_tuning()
        self._setup_models_and_optimizer()
        self._setup_storage()

    def _register_storage(self, obs_widths, extra_keys=()):
        """the rollout buffer — observation groups with a tail slab, the keys every update reads, `extra_keys` {name: width} — and the scratch
        buffers of GAE, sampling and the loss kernel"""
        T, N = self.num_steps_per_env, self.env.num_envs
        if not hasattr(self.env, "globals") or not hasattr(self.env, "set_obs_outputs"):
            raise _lib.PbhcError(f"pbhc_amd {type(self).__name__} drives the fused pbhc_amd env (needs env.globals / env.set_obs_outputs)")
        st = self.storage = RolloutStorage(N, T, self.device)
        for k, w in obs_widths.items():
            st.register_key(k, shape=(w,), dtype=torch.float, pad_rows=True, tail_slab=True)
        A, R = self.num_act, self.num_rew_fn
        for k, w, dt in [("actions", A, torch.float), ("rewards", R, torch.float), ("dones", 1, torch.bool), ("values", R, torch.float), ("returns", R, torch.float),
                         ("advantages", 1, torch.float), ("actions_log_prob", 1, torch.float), ("action_mean", A, torch.float), ("action_sigma", A, torch.float),
                         *((k, w, torch.float) for k, w in dict(extra_keys).items())]:
            st.register_key(k, shape=(w,), dtype=dt)
        self._gae_stats = torch.zeros(2 * ((T * N + 255) // 256) + 4, dtype=torch.float64, device=self.device)
        self._last_obs = {k: st.with_tail(k)[T] for k in obs_widths}      # the observations after the last step: slab T of the same buffers
        self._sample_seed = pdist.rank_seed(int(torch.randint(0, 2**62, (1,)).item()))
        self._branch_stream = torch.cuda.Stream(device=self.device)
        self._mb = (T * N) // self.num_mini_batches
        self._loss_scratch = torch.zeros(_lib.lib().pbhc_ppo_loss_scratch_floats(self._mb), device=self.device)
        self._grad_mu = torch.zeros(self._mb, A, device=self.device)
        self._grad_value = torch.zeros(self._mb, R, device=self.device)

    # ---- learn loop (mh_ppo.py:206-250, ppo_mimic.py:267-357) --------------------------------
    def _learn_loop(self, num_iterations, rollout, train, before_iteration=None):
        if self.__dict__.pop("_resume_in_loop", False):
            # a training state written inside this loop (`model_{it}.pt`): the run that wrote it went straight on to iteration it + 1, from the
            # observations its last rollout left — no random episode lengths, no reset_all()
            obs_dict = self._last_obs
        else:
            if self.init_at_random_ep_len:
                self.env.episode_length_buf = torch.randint_like(self.env.episode_length_buf, high=int(self.env.max_episode_length))
            obs_dict = self.env.reset_all()
        self._train_mode()
        n = self.num_learning_iterations if num_iterations is None else num_iterations
        tot_iter = self.current_learning_iteration + n
        for it in range(self.current_learning_iteration, tot_iter):
            if before_iteration is not None:
                before_iteration(it)
            self._timer.start()
            obs_dict = rollout(obs_dict)                      # ends with _timer.split(): collection | learning
            loss_dict = train()
            self._timer.split()
            self._post_epoch_logging(dict(it=it, loss_dict=loss_dict, num_learning_iterations=n))
            if self.log_dir is not None and it % self.save_interval == 0 and self.rank == 0:
                self.current_learning_iteration = it
                self._save_point = ("in_loop", it + 1)
                try:
                    self.save(os.path.join(self.log_dir, f"model_{it}.pt"))
                finally:
                    self._save_point = None
            self.ep_infos.clear()
        self.current_learning_iteration = tot_iter
        if self.log_dir is not None and self.rank == 0:
            self.save(os.path.join(self.log_dir, f"model_{self.current_learning_iteration}.pt"))

    # ---- exact resume (DESIGN.md §8 "Exact resume") ---------------------------------------------
    def training_state(self):
        """Everything outside the reference's checkpoint dictionary that decides how training goes on, as tensors, numbers, strings, lists,
        dicts and None (the file stays loadable with torch.load(weights_only=True)): where the state was taken (`resume_point` "in_loop" —
        by `_learn_loop` after an iteration — or "after_loop") and the iteration that comes next, the env's state_dict(), the observations
        the last rollout left, the episode book-keeping, the counters and the four process-wide generators.  Draws from no generator and
        launches nothing that writes state."""
        if self.world_size > 1:
            raise NotImplementedError("algo.config.save_training_state with more than one rank: every rank owns an env shard, only rank 0 "
                                      "writes the checkpoint")
        point, nxt = self.__dict__.get("_save_point") or ("after_loop", int(self.current_learning_iteration))
        ts = dict(version=resume.STATE_VERSION, resume_point=point, next_iteration=int(nxt), num_envs=int(self.env.num_envs),
                  sample_seed=int(self._sample_seed), env=self.env.state_dict(), last_obs={k: v.clone() for k, v in self._last_obs.items()},
                  cur_reward_sum=self.cur_reward_sum.clone(), cur_episode_length=self.cur_episode_length.clone(), ep_stats=self._ep_stats.clone(),
                  tot_timesteps=int(self.tot_timesteps), tot_time=float(self.tot_time), rollouts_done=int(self.__dict__.get("_rollouts_done", 0)),
                  rng=rng_state.capture_globals(self.device))
        ts["agent"] = self._extra_training_state()
        return ts

    def _extra_training_state(self):
        """hook: what a subclass adds to the training state ({name: tensor / number}); `_load_extra_training_state` takes it back"""
        return {}

    def _check_extra_training_state(self, extra):
        pass

    def _load_extra_training_state(self, extra):
        pass

    def check_training_state(self, ts):
        """everything `load_training_state` would refuse, without writing anything"""
        what = f"{type(self).__name__}.load_training_state"
        resume.check_version(ts, what)
        if ts["resume_point"] not in resume.RESUME_POINTS:
            raise _lib.PbhcError(f"{what}: resume_point {ts['resume_point']!r} is none of {resume.RESUME_POINTS}")
        resume.check_equal(what, "num_envs", int(ts["num_envs"]), int(self.env.num_envs))
        resume.check_equal(what, "the sampler's Philox key `_sample_seed` (seed torch with the saving run's config.seed before building env and agent)",
                           int(ts["sample_seed"]), int(self._sample_seed))
        resume.check_tensors(what, ts["last_obs"], self._last_obs)
        resume.check_tensors(what, ts, {"cur_reward_sum": self.cur_reward_sum, "cur_episode_length": self.cur_episode_length, "ep_stats": self._ep_stats})
        self.env.check_state_dict(ts["env"])
        self._check_extra_training_state(ts["agent"])

    def load_training_state(self, ts):
        """Take a `training_state()` back, after the weights and the optimiser: tensors in place, counters, generators last.  A state taken
        "in_loop" makes the next learn() skip its preamble and start at `next_iteration` from the restored observations."""
        if self.world_size > 1:
            raise NotImplementedError("algo.config.load_training_state with more than one rank: the training state holds ONE env shard")
        self.check_training_state(ts)
        self.env.load_state_dict(ts["env"])
        resume.restore(ts["last_obs"], self._last_obs)
        resume.restore(ts, {"cur_reward_sum": self.cur_reward_sum, "cur_episode_length": self.cur_episode_length, "ep_stats": self._ep_stats})
        self.tot_timesteps, self.tot_time = int(ts["tot_timesteps"]), float(ts["tot_time"])
        self._rollouts_done = int(ts["rollouts_done"])            # paces update_start_sampling (NOT the gate of the first graph capture)
        self.current_learning_iteration = int(ts["next_iteration"])
        self._resume_in_loop = ts["resume_point"] == "in_loop"
        self._load_extra_training_state(ts["agent"])
        rng_state.restore_globals(ts["rng"], self.device)

    def _with_training_state(self, ckpt):
        """save(): the reference's dictionary, + ONE key "training_state" when algo.config.save_training_state is true"""
        if self.config.get("save_training_state", False):
            ckpt["training_state"] = self.training_state()
        return ckpt

    def _restore_training_state(self, ckpt):
        """load(), after the weights and the optimiser: the file's training state, unless algo.config.load_training_state is false"""
        ts = ckpt.get("training_state", None)
        if ts is not None and self.config.get("load_training_state", True) is not False:
            self.load_training_state(ts)

    def _compute_returns(self, last_obs_dict, last_values=None):
        """mh_ppo.py:348-395 / ppo_mimic.py:443-491 in one HIP pass over the [T,N,R] slab."""
        st = self.storage
        if last_values is None:
            last_values = self._critic_values(last_obs_dict).detach()
        last_values = last_values.contiguous()
        T, N, R = self.num_steps_per_env, self.env.num_envs, self.num_rew_fn
        adv = st.advantages
        _lib.check(_lib.lib().pbhc_gae(st.rewards.data_ptr(), st.values.data_ptr(), st.dones.data_ptr(), last_values.data_ptr(), T, N, R,
                                       float(self.gamma), float(self.lam), st.returns.data_ptr(), adv.data_ptr(), self._gae_stats.data_ptr(),
                                       _lib.current_stream()), "pbhc_gae")
        if self._dp:
            # same normalisation as one big batch: undo the local one, re-normalise with global moments
            nb = (T * N + 255) // 256
            mean_l, std_l = self._gae_stats[2 * nb].float(), self._gae_stats[2 * nb + 1].float()
            adv.copy_(pdist.global_normalize_(adv * (std_l + 1e-8) + mean_l))
        return st.returns, adv

    # ---- the frame of `_training_step` -------------------------------------------------------
    def _begin_meters(self, names, summed=None):
        """-> (meters, loss): one fill — a meter per name and, behind them, the loss kernel's running sums {surrogate, value, entropy, kl}
        (`loss["_acc"]`); `loss` holds the first `summed` meters (the ones an optimiser step adds to)"""
        meters = torch.zeros(len(names) + 4, device=self.device)
        loss = {k: meters[i] for i, k in enumerate(names[:summed])}
        loss["_acc"] = meters[len(names):]
        return meters, loss

    def _end_meters(self, names, meters, loss):
        acc = loss.pop("_acc")
        loss["Surrogate"] += acc[0]; loss["Value"] += acc[1]; loss["Entropy"] += acc[2]
        self.storage.clear()
        means = meters[:len(names)] / (self.num_learning_epochs * self.num_mini_batches)
        return {k: means[i] for i, k in enumerate(names)}

    # ---- evaluation / export surface --------------------------------------------------------
    def get_example_obs(self):
        obs = self.env.reset_all()
        return {k: v.clone() for k, v in obs.items()}

    # ---- logging (mh_ppo.py:547-700, reduced to the Perf/* + Loss/* + Train/* scalars) ------
    def _post_epoch_logging(self, log):
        self.tot_timesteps += self.num_steps_per_env * self.env.num_envs * self.world_size
        if log["it"] % self.logging_interval != 0:
            return
        for c, l in self._timer.resolve():                  # device time of every iteration since the last logging interval
            self.collection_time, self.learn_time = c, l
            self.tot_time += c + l
        log["collection_time"], log["learn_time"] = self.collection_time, self.learn_time
        it_time = self.collection_time + self.learn_time
        if self.rank != 0:
            return
        stats = self._ep_stats.tolist()           # the only read-back, once per logging interval
        self._ep_stats.zero_()
        fps = int(self.num_steps_per_env * self.env.num_envs * self.world_size / max(it_time, 1e-9))
        it, w = log["it"], self.writer
        for k, v in log["loss_dict"].items():
            w.add_scalar("Loss/" + k, float(v), it)
        self._log_scalars(w, it)
        w.add_scalar("Perf/total_fps", fps, it)
        w.add_scalar("Perf/collection_time", log["collection_time"], it)
        w.add_scalar("Perf/learning_time", log["learn_time"], it)
        if stats[2] > 0:
            w.add_scalar("Train/mean_reward", stats[0] / stats[2], it)
            w.add_scalar("Train/mean_episode_length", stats[1] / stats[2], it)
        for k, v in (self.env.read_log() if hasattr(self.env, "read_log") else {}).items():
            w.add_scalar("Env/" + k, float(v), it)
        print(f"[it {it}] fps {fps}  collect {log['collection_time']:.3f}s  learn {log['learn_time']:.3f}s  {self._log_line(log['loss_dict'])}  "
              f"ep_rew {stats[0] / max(stats[2], 1):.3f}  ep_len {stats[1] / max(stats[2], 1):.1f}", flush=True)
